"""ca_copy_number_profile on the device: per (gene or block of genes, clone, candidate copy number) the sum over the clone's cells of total log1p(a), a = the
relative change of the cell's normaliser.  Oracle: the float64 numpy restatement on whole arrays of tests/_copy_number_profile_cases.py (``numpy_cost``).
Scale per entry: sum_n s_n (|log1p(a)| + |a| / (1 + a)), the conditioning of log1p; bars 1e-10 of it (parity) and 1e-12 of it (splits and batch cuts); an
entry where the restatement has 1 + a == 0 is compared for -inf exactly, and -inf is accepted nowhere else."""
import ctypes

import numpy as np
import pytest

from clonealign_amd import api, engine

from tests import _copy_number_profile_cases as cc
from tests import _simulate_cases as sc

pytestmark = pytest.mark.gpu
RTOL = 1e-10
KAPPA3 = np.array([0.0, 1.0, 2.5])
KAPPA6 = np.array([0.0, 1.0, 2.0, 3.0, 4.0, 6.5])
KAPPA16 = np.r_[0.0, 0.25, np.linspace(0.5, 7.0, 14)]


def compare(got, want, scale, rtol, what):
    """The largest |got - want| / scale over the finite entries; asserts that ``got`` is -inf exactly where ``want`` is (the restatement has 1 + a == 0 for a
    cell of the entry) and within ``rtol * scale`` everywhere else."""
    assert got.shape == want.shape and got.dtype == np.float64 and not np.isnan(got).any(), what
    exact = np.isneginf(want)
    assert not np.isposinf(want).any() and np.array_equal(np.isinf(got), exact) and (got[exact] == -np.inf).all(), what
    diff = np.abs(got[~exact] - want[~exact])
    worst = float(np.max(diff / np.where(scale[~exact] > 0, scale[~exact], 1.0), initial=0.0))
    bad = diff > rtol * scale[~exact]
    assert not bad.any(), (what, worst, int(bad.sum()))
    return worst


def labellings(G):
    return {"per gene": None, "contiguous": (np.arange(G) * min(G, 12) // G).astype(np.int32), "interleaved": (np.arange(G) % 7 % G).astype(np.int32),
            "one block": np.zeros(G, dtype=np.int32)}


def case_mu(name):
    E = sc.make(name)[0]
    return np.random.default_rng(4000 + sorted(sc.CASES).index(name)).lognormal(0.0, 1.0, E.shape[0])


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_parity_with_the_numpy_restatement(name):
    """Every case of _simulate_cases.CASES: ragged tiles, E = 0 in places with totals 0 / 1 / 200 000 (`mixed`), twenty clones at G = 2049, 20 000 genes (the
    row of w in the block's global slab), three genes, |eta| = 700 (`steep`).  mu ~ lognormal(0, 1) per case; kappa = (0, 1, 2.5), (0, 1, 2, 3, 4, 6.5) and a
    grid of 16 (the J buckets 4, 8 and 16); per-gene mode and block mode under a contiguous, an interleaved (g % 7) and a single-block labelling.  Bar: 1e-10
    scale; -inf exactly where the restatement has it (`ragged` and `few_genes` have D = 0: the library's host path).
    Largest ratios measured on an MI355X over the cases with factors: per gene 3.4e-16 (`pow2_plus_1`) and 1.4e-14 at `steep` (where
    5 entries are -inf on both sides: the top gene's p rounds to 1); block mode 1.2e-13 (`pow2_plus_1`, contiguous), 1.0e-13 (`pow2_plus_1`, interleaved),
    7.0e-14 (`large_g`), 4.8e-14 (`steep`), below 2.7e-14 elsewhere; the bucket of 4 (J = 3) 1.4e-14 per gene and 1.2e-13 in block mode, at the same cases."""
    E, V, U, clone, total, _seed = sc.make(name)
    mu = case_mu(name)
    for kappa in (KAPPA3, KAPPA6, KAPPA16):
        for label, blocks in labellings(E.shape[0]).items():
            got = engine.copy_number_profile(E, V, U, clone, total, mu, kappa, blocks=blocks)
            worst = compare(got, *cc.numpy_cost(E, V, U, clone, total, mu, kappa, blocks), RTOL, (name, label, kappa.shape[0]))
            print(f"{name}, J = {kappa.shape[0]}, {label}: largest |device - numpy| / scale = {worst:.2e}; {int(np.isneginf(got).sum())} entries -inf")
            assert (engine.copy_number_profile_kernel_ms() > 0.0) == (U is not None)


def test_determinism_and_splits():
    """`mixed`, split at 137, per-gene mode and the interleaved blocks: two calls agree bit for bit; the two calls on [0, 137) and [137, N) add up to the one
    call's table within 1e-12 scale.  Measured on an MI355X: 4.2e-16 per gene, 2.8e-16 with blocks."""
    E, V, U, clone, total, _seed = sc.make("mixed")
    mu, h = case_mu("mixed"), 137
    for blocks in (None, labellings(E.shape[0])["interleaved"]):
        one, again = (engine.copy_number_profile(E, V, U, clone, total, mu, KAPPA6, blocks=blocks) for _ in range(2))
        assert np.array_equal(one, again)
        lo = engine.copy_number_profile(E, V, U[:h], clone[:h], total[:h], mu, KAPPA6, blocks=blocks)
        hi = engine.copy_number_profile(E, V, U[h:], clone[h:], total[h:], mu, KAPPA6, blocks=blocks)
        _want, scale = cc.numpy_cost(E, V, U, clone, total, mu, KAPPA6, blocks)
        worst = compare(lo + hi, one, scale, 1e-12, "split")
        print(f"split at {h}, {'blocks' if blocks is not None else 'per gene'}: largest |lo + hi - one| / scale = {worst:.2e}")


@pytest.mark.parametrize("by_block", [False, True])
def test_a_batch_cut_changes_nothing_beyond_rounding(by_block):
    """The recipe of test_batches_of_cells_change_no_bit: G = 9, D = 1; a batch holds 64 MB / (8 D + 56) = 1 048 576 cells per gene and, with B = 3 blocks, 64 MB
    / (8 D + 56 + 16 B) = 599 186 cells; N is 24 cells more, so the call goes as two batches; all but 30 cells at the ends and around the cut have total 0.
    The 30 cells alone give the same table within 1e-12 scale.  Measured on an MI355X: 1.4e-16 per gene (cut at 1 048 576), 1.7e-16 with blocks (cut at 599 186)."""
    rng = np.random.default_rng(8)
    G, C = 9, 2
    blocks = (np.arange(G) % 3).astype(np.int32) if by_block else None
    cut = (64 << 20) // (8 + 56 + (16 * 3 if by_block else 0))
    N = cut + 24
    E = rng.lognormal(0.0, 1.0, (G, 1)) * rng.integers(1, 5, (G, C)).astype(np.float64)
    mu = rng.lognormal(0.0, 1.0, G)
    V = rng.normal(size=(G, 1)) * 0.5
    U = rng.normal(size=(N, 1))
    clone = rng.integers(0, C, N).astype(np.int32)
    total = np.zeros(N, dtype=np.int64)
    cells = np.r_[0:6, cut - 6:cut + 6, N - 12:N]
    total[cells] = rng.integers(1, 300, cells.size)
    one = engine.copy_number_profile(E, V, U, clone, total, mu, KAPPA6, blocks=blocks)
    few = engine.copy_number_profile(E, V, U[cells], clone[cells], total[cells], mu, KAPPA6, blocks=blocks)
    want, scale = cc.numpy_cost(E, V, U[cells], clone[cells], total[cells], mu, KAPPA6, blocks)
    compare(few, want, scale, RTOL, "the 30 cells")
    worst = compare(one, few, scale, 1e-12, "batch cut")
    print(f"batch cut at {cut}, {'blocks' if by_block else 'per gene'}: largest |all cells - the 30 cells| / scale = {worst:.2e}")


def test_exact_zeros_and_minus_infinity_on_the_device():
    for what, args, Lint in cc.exact_cases():
        cc.check_exact(lambda E, V, U, clone, total, mu, kappa, blocks: engine.copy_number_profile(E, V, U, clone, total, mu, kappa, blocks=blocks), what, args, Lint)


def test_refusals_name_the_argument_and_leave_cost_alone():
    E, _V, _U, clone, total, _seed = sc.make("ragged")
    N, G, C = clone.shape[0], E.shape[0], E.shape[1]
    V, U = np.zeros((G, 1)), np.zeros((N, 1))
    mu, kappa, labels = np.ones(G), np.arange(4.0), (np.arange(G) % 5).astype(np.int32)
    lib, err = engine.load_library(), ctypes.create_string_buffer(256)
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731

    def poke(a, idx, v):
        b = np.array(a, dtype=np.float64 if a.dtype.kind == "f" else a.dtype)
        b[idx] = v
        return b

    def refused(match, E=E, V=V, U=U, clone=clone, total=total, D=1, mu=mu, kappa=kappa, J=None, B=G, labels=None, null_cost=False):
        cost = np.full(4096 * C * 17, -7.0)
        keep = [None if a is None else np.ascontiguousarray(a, dtype=t) for a, t in ((E, np.float64), (V, np.float64), (U, np.float64), (clone, np.int32),
                                                                                      (total, np.int64), (mu, np.float64), (kappa, np.float64), (labels, np.int32))]
        rc = lib.ca_copy_number_profile(N, G, C, D, *(ptr(a) for a in keep[:6]), len(kappa) if J is None else J, ptr(keep[6]), B, ptr(keep[7]), 0,
                                        None if null_cost else ptr(cost), err)
        assert rc == 1, match                                                                   # CA_ERR_INVALID
        assert err.value.startswith(b"ca_copy_number_profile: ") and match in err.value, err.value
        assert (cost == -7.0).all(), match
        assert engine.copy_number_profile_kernel_ms() == 0.0

    refused(b"mu has a negative", mu=poke(mu, 3, -1.0))
    refused(b"mu has a negative or non-finite entry (gene 5)", mu=poke(mu, 5, np.nan))
    refused(b"kappa has a negative or non-finite entry (candidate 2)", kappa=poke(kappa, 2, np.nan))
    refused(b"J = 0 is outside", J=0)
    refused(b"J = 17 is outside", kappa=np.arange(17.0))
    refused(b"block_of_gene[4] = 5 is outside [0, 5)", B=5, labels=poke(labels, 4, 5))
    refused(b"block_of_gene[7] = -1 is outside", B=5, labels=poke(labels, 7, -1))
    refused(b"block_of_gene is NULL (per-gene mode), where B must equal G", B=G - 1)
    refused(b"B = 2049 blocks; block mode takes at most 2048", B=2049, labels=labels)
    refused(b"per-gene mode", B=2049, labels=labels)
    refused(b"cost must not be NULL", null_cost=True)
    refused(b"mu and kappa must not be NULL", mu=None)
    refused(b"E has a negative", E=poke(E, (3, 1), -1.0))
    refused(b"U has a non-finite", U=poke(U, (5, 0), np.nan))
    refused(b"V has a non-finite", V=poke(V, (76, 0), np.nan))
    refused(b"clone[4] = 2 is outside", clone=poke(clone, 4, C))
    refused(b"total[2] = -1 is outside", total=poke(total, 2, -1))
    refused(b"but E is zero in every gene of the cell's clone 1", E=np.column_stack([E[:, 0], np.zeros(G)]))
    refused(b"D = 9 is outside", V=np.zeros((G, 9)), U=np.zeros((N, 9)), D=9)
    refused(b"needs both U", U=None)
    with pytest.raises(engine.EngineError, match=r"ca_copy_number_profile: mu has a negative"):
        engine.copy_number_profile(E, V, U, clone, total, poke(mu, 3, -1.0), kappa)
    # no cells: zeros; and after a call that ran kernels a refusal leaves the time at 0
    for blocks in (None, labels):
        empty = engine.copy_number_profile(E, V, U[:0], clone[:0], total[:0], mu, kappa, blocks=blocks)
        assert empty.shape == (G if blocks is None else 5, C, 4) and (empty == 0.0).all()
    engine.copy_number_profile(E, V, U, clone, total, mu, kappa)
    assert engine.copy_number_profile_kernel_ms() > 0.0
    refused(b"J = 0 is outside", J=0)


def test_python_on_the_device():
    """The planted case of tests/_copy_number_profile_cases.py (240 x 300 x 3, 12 segments, four corrupted (segment, clone) entries), dense and CSR:
    host=False equals host=True within 1e-10 scale (cost and delta_ll), T_observed bit for bit; the recovery is the host test's; then the rules of delta_ll
    on ``rules_case``.  Measured on an MI355X: block-mode log_bf of the four corrupted entries 388 .. 1398; per gene recovered 0.934 of 106, kept 0.965 of
    794, dense and CSR alike."""
    import scipy.sparse as sp
    fit, Y, L_given, L_true, seg, bad, z = cc.planted()
    blk_h, gene_h = cc.check_planted(fit, Y, L_given, L_true, seg, bad, host=True)
    ml, cand = fit["ml_params"], np.arange(1.0, 7.0)
    bg = api._block_labels(seg, 300)[1]
    scales = {False: cc.numpy_cost(ml["mu"][:, None] * L_given, ml["W"], ml["psi"], z, Y.sum(1), ml["mu"], cand)[1],
              True: cc.numpy_cost(ml["mu"][:, None] * L_given, ml["W"], ml["psi"], z, Y.sum(1), ml["mu"], cand, bg)[1]}
    for Yd in (Y, sp.csr_matrix(Y)):
        blk_d, gene_d = cc.check_planted(fit, Yd, L_given, L_true, seg, bad)
        for by_block, dev, hst in ((True, blk_d, blk_h), (False, gene_d, gene_h)):
            assert np.array_equal(dev["T_observed"], hst["T_observed"]) and np.array_equal(dev["gain"], hst["gain"])
            scale = scales[by_block]
            assert np.isfinite(dev["cost"]).all() and (np.abs(dev["cost"] - hst["cost"]) <= RTOL * scale).all()
            assert (np.abs(dev["delta_ll"] - hst["delta_ll"]) <= RTOL * scale).all()
            assert np.array_equal(dev["map_cn"], hst["map_cn"]) and np.array_equal(dev["input_cn"], hst["input_cn"])
    fit_r, Y_r, L_r, z_r, planted_read = cc.rules_case()
    cc.check_rules(api.copy_number_profile(fit_r, Y_r, L_r), Y_r, L_r, z_r, planted_read, "device")
