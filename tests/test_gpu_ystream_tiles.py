"""The count-matrix stream's staging tiles (clonealign_amd/csrc/ca_ymfma.hip.h, round 19): a wave parks each 64-cell x 64-gene piece in LDS as four cell tiles
of 16 rows, CA_YS_TILE bytes apart, and reads them back row-wise (1-byte image) and transposed (every image).  A wrong tile base sums the wrong cells into a
gene, or the wrong genes into a cell, so the matrix here gives every (cell tile, gene tile) pair of a piece its own count rate: no two tiles of a piece can be
exchanged without moving YW and Y^T psi by far more than any tolerance below.

YWpart / YTpart come out through HipEngine.ystream_parts (ca_ystream_parts: the two float slabs as the last launch left them, the exponents it read, the
fixed-point values in the quantiser's images); the finished sums through the gradients, as in tests/test_gpu_y4.py and tests/test_gpu_y2.py: d ELBO / d psi holds
(Y W)_n and d ELBO / d W holds (Y^T psi)_g, everything else in them comes from launches that never see the stream's LDS.

* exact: the slabs equal int64 numpy products of the counts (min(y, 255): the resident byte; the excess goes through the overflow list, outside the slabs) with
  the quantiser's own fixed-point values, scaled by 2^-exponent in float64 (exact: the integers stay below 2^53) and rounded to float32 once, as the kernel
  does -- np.array_equal, every image, every position of the moment role, both shapes.  The only reference here that never went through the staging tiles;
* bit-equal between the 1-byte, the 4-bit and the 2-bit / 4-bit image, and between the moment role in front of the stream's blocks, behind them and off
  (np.array_equal on slabs, gradients, ELBOs and states): integer sums do not depend on the image or on which launch form carries them;
* the finished gradients against float64 (tests/_series_ref.ref_gradients), per element, at the per-element tolerances of tests/test_gpu_series_grad.py
  (W 1.19e-6, psi 9.52e-7 of the summands' magnitudes): the finisher and the launches behind it, which the slabs do not cover.

Measured on an MI355X (largest |engine - float64| / scale over all elements, the same for the three images): 200 x 1100: W 7.82e-08, psi 2.96e-08;
64 x 512: W 6.95e-08, psi 2.25e-08.  With the transposed reads of odd tiles at the even tiles' bank offset, or at the plain pitch: W 18 .. 296; with psi's mask index
off by one: W 2.9 .. 13 in the 4-bit forms (profiles/r19_stream_ab.txt (D)).

Shapes: 200 x 1100 x 4 (all four cell tiles live in three full 64-cell steps, a last step of 8 cells, several segments with a ragged last one) and 64 x 512 x 4
(one step, one row group).  A wave's strip is 64 cells at both, so each wave runs one step; all eight gene blocks of a segment and the narrow and wide pieces
of the 2-bit / 4-bit image (N2 = 6) are live."""
import numpy as np
import pytest

from tests import _series_ref as sr
from tests._cases import eps_for, make_case

pytestmark = pytest.mark.gpu

TOL = {"W": 8.0 * 1.482e-07, "psi": 8.0 * 1.190e-07}      # tests/test_gpu_series_grad.py: TOL = 8 x its OBSERVED, per element against the summands' magnitudes
IMAGES = {"y2": (("series", "y2"), (), 4, 6), "y4": (("series", "y4"), ("y2",), 4, 0), "u8": (("series",), ("y2", "y4"), 8, 0)}
ROLES = {"behind": (("mom_last",), ()), "front": ((), ("mom_last",)), "off": ((), ("mom_ride",))}
SHAPES = [(200, 1100), (64, 512)]


def _planted(N, G, seed):
    """Poisson counts whose rate is set by the (cell tile, gene tile) pair: 0.15 + 0.1 (4 ct + gt), ct = (n >> 4) & 3, gt = (g >> 4) & 3 -- sixteen rates from
    0.15 to 1.65, so the sixteen tiles of every piece carry different sums.  One gene in sixteen is busy (rate 6: the wide blocks of the 2-bit / 4-bit image),
    a few counts reach 15 .. 40 anywhere (the 4-bit escape list; in quiet genes the 2-bit one, which the Poisson tail from 3 up fills as well) and three exceed
    255 (the overflow list)."""
    rng = np.random.default_rng(seed)
    n, g = np.arange(N)[:, None], np.arange(G)[None, :]
    lam = 0.15 + 0.1 * (4 * ((n >> 4) & 3) + ((g >> 4) & 3))
    Y = rng.poisson(lam).astype(np.float64)
    busy = np.flatnonzero(rng.random(G) < 1.0 / 16.0)
    Y[:, busy] = rng.poisson(6.0, size=(N, busy.size))
    flat = rng.choice(Y.size, Y.size // 500, replace=False)
    Y.flat[flat] = rng.integers(15, 41, size=flat.size)
    Y.flat[rng.choice(Y.size, 3, replace=False)] = (256, 300, 411)
    Y[:, 0] += 1
    Y[0, :] += 1
    assert (Y > 255).sum() >= 3 and (Y >= 15).sum() > 20
    return Y


_RUNS = {}


def _runs(N, G):
    """Every (image, role) engine of a shape once: the gradients at the start state through the plain call, then one iteration of the loop (the series form's
    launches, the moment role where it rides), the gradients its update applied and the state after it."""
    if (N, G) in _RUNS:
        return _RUNS[(N, G)]
    from clonealign_amd.engine import HipEngine
    Y = _planted(N, G, 1000 + N)
    c = make_case(N=8, G=G, C=4, K=1, seed=3)
    rng = np.random.default_rng(7)
    case = dict(Y=Y, L=c["L"], psi0=rng.normal(size=(N, 1)), loc0=c["loc0"], K=1, S=1)
    W0 = rng.uniform(-0.3, 0.3, size=(G, 1))
    e0 = eps_for(1, G, 5)
    eps = np.stack([eps_for(1, G, 900 + i) for i in range(2)])
    out = {"Y": Y, "L": c["L"], "eps": eps}
    for img, (on, off, bits, n2) in IMAGES.items():
        for role, (r_on, r_off) in ROLES.items():
            eng = HipEngine(**case, variant_on=on + r_on, variant_off=off + r_off)
            try:
                eng.set("W", W0)
                i0 = eng.info()
                assert i0["fwd_series"] == 1 and (i0["y_stream_bits"], i0["y_stream_n2"]) == (bits, n2), (img, role, i0)
                assert (i0["mom_ride"], i0["mom_last"]) == {"behind": (1, 1), "front": (1, 0), "off": (0, 0)}[role], (img, role, i0["mom_ride"], i0["mom_last"])
                if bits == 4:
                    assert i0["y_stream_esc"] > 0, i0      # the image's escape list is non-empty
                g, e = eng.gradients(e0)      # (the parameters were just set: this pass launches the stream, the moment role with it)
                p0 = eng.ystream_parts()
                s0 = eng.get_state()
                el = eng.iterate(1, eps)
                p1 = eng.ystream_parts()
                i1 = eng.info()
                assert i1["series_passes"] - i0["series_passes"] >= 1 and i1["series_fallbacks"] == i0["series_fallbacks"], (img, role, i1)
                out[(img, role)] = dict(grad=g, elbo0=e, s0=s0, elbo1=el, last=eng.last_gradients(("W", "psi")), s1=eng.get_state(), p0=p0, p1=p1)
            finally:
                eng.close()
    _RUNS[(N, G)] = out
    return out


def _same(a, b, what):
    assert a["elbo0"] == b["elbo0"] and a["elbo1"] == b["elbo1"], (what, a["elbo0"], b["elbo0"], a["elbo1"], b["elbo1"])
    for part in ("grad", "last", "s1", "p0", "p1"):
        assert set(a[part]) == set(b[part])
        for k in a[part]:
            assert np.array_equal(a[part][k], b[part][k], equal_nan=True), (what, part, k)


def _fix(x, e):
    """The quantiser's fixed-point value of a float32 entry (ca_ys_quant_core): rint(x 2^e) in float32 -- the product is exact, rint rounds half to even."""
    return np.rint(np.clip(np.asarray(x, np.float64).astype(np.float32) * np.float32(2.0 ** int(e)), -2147483000.0, 2147483000.0)).astype(np.int64)


def _slabs(Y, parts):
    """YWpart [nseg][N] and YTpart [nrg][Gp] from the counts and the fixed-point values in `parts`: int64 products, one rounding to float32."""
    N, G = Y.shape
    nseg, nrg = parts["yw_part"].shape[0], parts["yt_part"].shape[0]
    Gp, rows = parts["yt_part"].shape[1], 4 * parts["strip_cells"]
    assert Gp == 512 * nseg and nrg == -(-N // rows)
    Yc = np.zeros((nrg * rows, Gp), np.int64)
    Yc[:N, :G] = np.minimum(Y, 255.0).astype(np.int64)
    wf = parts["w_fix"].astype(np.int64)
    pf = np.zeros(nrg * rows, np.int64)
    pf[:N] = parts["p_fix"][:N]
    yw = np.stack([Yc[:N, 512 * s:512 * (s + 1)] @ wf[512 * s:512 * (s + 1)] for s in range(nseg)])
    yt = np.stack([pf[rows * r:rows * (r + 1)] @ Yc[rows * r:rows * (r + 1)] for r in range(nrg)])
    assert max(np.abs(yw).max(), np.abs(yt).max()) < 2 ** 53
    ew, ep = (int(x) for x in parts["exps"])
    return (yw.astype(np.float64) * 2.0 ** -ew).astype(np.float32), (yt.astype(np.float64) * 2.0 ** -ep).astype(np.float32)


@pytest.mark.parametrize("N,G", SHAPES)
def test_tiles_slabs_equal_int64_products_with_the_quantisers_values(N, G):
    """YWpart / YTpart of the launch that ca_gradients made (own launch, moment role where it rides) against int64 numpy products, exactly.  After the loop's
    iteration the slabs are either a later launch's (its monitor pass: the images are current, the same check) or still these."""
    r = _runs(N, G)
    for img in IMAGES:
        for role in ROLES:
            run = r[(img, role)]
            p0, p1 = run["p0"], run["p1"]
            assert p0["images_current"], (img, role)
            # the images hold fix() of the state: the quantiser's values are the formula's, zero past G and N
            assert np.array_equal(p0["w_fix"][:G], _fix(run["s0"]["W"].reshape(-1), p0["exps"][0])) and not p0["w_fix"][G:].any(), (img, role)
            assert np.array_equal(p0["p_fix"][:N], _fix(run["s0"]["psi"].reshape(-1), p0["exps"][1])) and not p0["p_fix"][N:].any(), (img, role)
            assert np.abs(p0["w_fix"]).max() >= 2 ** 28 and np.abs(p0["p_fix"]).max() >= 2 ** 28      # all four digits of the images are live
            yw, yt = _slabs(r["Y"], p0)
            nbad = (int((yw != p0["yw_part"]).sum()), int((yt != p0["yt_part"]).sum()))
            print(f"ystream_tiles exact {N}x{G} {img} {role}: YWpart {nbad[0]} of {yw.size} differ, YTpart {nbad[1]} of {yt.size}")
            assert np.array_equal(yw, p0["yw_part"]) and np.array_equal(yt, p0["yt_part"]), (img, role, nbad)
            if p1["images_current"]:
                yw1, yt1 = _slabs(r["Y"], p1)
                assert np.array_equal(yw1, p1["yw_part"]) and np.array_equal(yt1, p1["yt_part"]), (img, role, "after the iteration")
            else:
                assert np.array_equal(p1["yw_part"], p0["yw_part"]) and np.array_equal(p1["yt_part"], p0["yt_part"]), (img, role, "no launch since")


@pytest.mark.parametrize("N,G", SHAPES)
def test_tiles_bit_equal_between_the_images(N, G):
    r = _runs(N, G)
    for role in ROLES:
        for img in ("y2", "y4"):
            _same(r[(img, role)], r[("u8", role)], (img, role))


@pytest.mark.parametrize("N,G", SHAPES)
def test_tiles_bit_equal_between_the_moment_roles(N, G):
    r = _runs(N, G)
    for img in IMAGES:
        for role in ("behind", "front"):
            _same(r[(img, role)], r[(img, "off")], (img, role))


@pytest.mark.parametrize("N,G", SHAPES)
def test_tiles_match_float64_products_of_the_counts(N, G):
    """d ELBO / d W and d ELBO / d psi the loop's update applied (the finished sums), against float64 with Y^T psi and Y W as numpy products, per element."""
    r = _runs(N, G)
    fc = sr.fit_constants(r["Y"], r["L"])
    worst = {}
    for img in IMAGES:
        run = r[(img, "behind")]
        ref, sc = sr.ref_gradients(fc, run["s0"], r["eps"][0][0])
        for k in ("W", "psi"):
            worst[(img, k)] = sr.worst_ratio(run["last"][k], ref[k], sc[k])
            print(f"ystream_tiles {N}x{G} {img} {k} {worst[(img, k)]:.3e}")
    bad = {k: v for k, v in worst.items() if not v <= TOL[k[1]]}
    assert not bad, bad
