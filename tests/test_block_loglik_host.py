"""clone_loglik_by_block / assignment_support on the host (float64 numpy only): the split of the multinomial log-likelihood over blocks of genes.

The yardsticks are ``_clone_loglik_host`` (the chunked float64 host form of ``clone_loglik``) and ``ref_ll`` of tests/test_gpu_clone_loglik.py on the
RESTRICTED matrices: ``without[:, b]`` must be the log-likelihood of the problem with block b's columns deleted, ``within[:, b]`` the one of block b's
columns alone, and ``sum_b within + between`` the one of the whole matrix.  Bar: the project's float64 bar, ``1e-10 x`` the sum of the terms' magnitudes
(``scale`` of ``ref_ll`` on the same restricted matrices)."""
import numpy as np
import pytest

import clonealign_amd as ca
from clonealign_amd import api
from tests._cases import make_case
from tests.test_gpu_clone_loglik import ref_ll

RTOL = 1e-10
CUTS = (1, 17, 130, 255, 257, 513, 1023, 1025, 2048)


def contiguous_labels(G):
    """Blocks of consecutive genes cut at CUTS (those inside (0, G)): (block_of_gene, n_blocks)."""
    cuts = np.array([c for c in CUTS if 0 < c < G], dtype=np.int64)
    return np.searchsorted(cuts, np.arange(G), side="right").astype(np.int32), int(cuts.size) + 1


def interleaved_labels(G):
    """``g % 5`` with 7 blocks: blocks 5 and 6 are empty."""
    return (np.arange(G) % 5).astype(np.int32), 7


LABELLINGS = {"contiguous": contiguous_labels, "mod5of7": interleaved_labels}


def close(out, ref, scale, tag):
    """``out`` against ``ref`` at the bar: the same -inf pattern, no NaN, finite entries within RTOL x scale (a scale of 0 asks for equality)."""
    assert out.shape == ref.shape, tag
    assert not np.isnan(out).any(), tag
    assert np.array_equal(np.isneginf(out), np.isneginf(ref)), tag
    ok = np.isfinite(ref)
    assert np.isfinite(out[ok]).all(), tag
    err = np.abs(out[ok] - ref[ok])
    assert (err <= RTOL * scale[ok]).all(), (tag, float((err / np.maximum(scale[ok], 1e-300)).max()))


def restricted(Y, E, U, V, keep, const):
    """(ll, scale) of the problem restricted to the genes ``keep``; no gene: 0 for every cell and clone."""
    if keep.size == 0:
        z = np.zeros((Y.shape[0], E.shape[1]))
        return z, z
    with np.errstate(divide="ignore", invalid="ignore"):            # (a clone absent from every kept gene: ref_ll forms log 0)
        return ref_ll(Y[:, keep], E[keep], U, None if V is None else V[keep], const=const)


def check_terms(terms, Y, E, U, V, bg, B, const, tag):
    """The three identities of the module docstring, block by block."""
    full, fscale = ref_ll(Y, E, U, V, const=const)
    close(terms["clone_loglik"], full, fscale, tag + " total")
    for b in range(B):
        inb = np.flatnonzero(bg == b)
        out = np.flatnonzero(bg != b)
        close(terms["without"][:, b], *restricted(Y, E, U, V, out, const), f"{tag} without {b}")
        ref, scale = restricted(Y, E, U, V, inb, const)
        if inb.size and (E[inb].sum(0) == 0).any():                  # (a clone absent from the whole block: its cells without counts there give 0)
            sb = Y[:, inb].sum(1)
            ref = np.where((sb == 0)[:, None], 0.0, np.where(np.isnan(ref), -np.inf, ref))
            scale = np.where(np.isfinite(scale), scale, 0.0)
        close(terms["within"][:, b], ref, scale, f"{tag} within {b}")
        assert (terms["within"][:, b][Y[:, inb].sum(1) == 0] == 0.0).all(), tag


def host_terms(Y, E, U, V, bg, B, const):
    st = api._clone_loglik_by_block_host(Y, E, U, V, bg, B, const=const)
    return st, api._by_block_terms(st["A"], st["logZ"], st["s"], st["lg"])


def case_tables(N, G, C, D, seed):
    case = make_case(N=N, G=G, C=C, K=0, seed=seed)
    rng = np.random.default_rng(seed + 1)
    mu = rng.lognormal(0, 0.5, G)
    U, V = (rng.normal(size=(N, D)) * 0.5, rng.normal(size=(G, D)) * 0.3) if D else (None, None)
    return case["Y"], case["L"], mu, U, V, rng


@pytest.mark.parametrize("labelling", sorted(LABELLINGS))
@pytest.mark.parametrize("const", [True, False])
@pytest.mark.parametrize("D", [0, 2])
@pytest.mark.parametrize("shape", [(33, 77, 2), (300, 500, 5)], ids=lambda s: "x".join(map(str, s)))
def test_blocks_add_up_and_match_the_restricted_problems(shape, D, const, labelling):
    N, G, C = shape
    Y, L, mu, U, V, _rng = case_tables(N, G, C, D, seed=sum(shape) + D)
    E = mu[:, None] * L
    bg, B = LABELLINGS[labelling](G)
    st, terms = host_terms(Y, E, U, V, bg, B, const)
    assert st["A"].shape == st["logZ"].shape == (N, B, C) and st["s"].shape == (N, B) and (st["lg"] is None) == (not const)
    assert np.array_equal(st["s"].sum(1), Y.sum(1))
    # the host form of the whole matrix, as the issue names it, and then every block against the restricted problems
    whole = api._clone_loglik_host(Y, E, U, V, const=const)
    close(terms["clone_loglik"], whole, ref_ll(Y, E, U, V, const=const)[1], "against _clone_loglik_host")
    for b in range(B):
        keep = np.flatnonzero(bg != b)
        sub = api._clone_loglik_host(Y[:, keep], E[keep], U, None if V is None else V[keep], const=const)
        close(terms["without"][:, b], sub, restricted(Y, E, U, V, keep, const)[1], f"without {b} against _clone_loglik_host")
    check_terms(terms, Y, E, U, V, bg, B, const, f"{shape} D={D} const={const} {labelling}")
    for b in range(B):                                               # an empty block: nothing within, nothing missing without
        if not (bg == b).any():
            assert (st["A"][:, b] == 0).all() and (st["s"][:, b] == 0).all() and np.isneginf(st["logZ"][:, b]).all()
            assert (terms["within"][:, b] == 0).all()
            assert np.array_equal(terms["without"][:, b], terms["without"][:, B - 1])    # (both empty: the same scans' result)


@pytest.mark.parametrize("D", [0, 2])
def test_zero_copy_number_gives_minus_infinity_where_the_restricted_problem_does(D):
    N, G, C = 300, 500, 5
    Y, L, mu, U, V, _rng = case_tables(N, G, C, D, seed=41)
    bg, B = contiguous_labels(G)
    g2 = int(np.flatnonzero(bg == 2)[3])                             # one gene of block 2 where clone 1 has no copy ...
    L[g2, 1] = 0.0
    Y[:, g2] = 0
    Y[7, g2] = 3                                                     # ... and one cell with counts there
    blk4 = np.flatnonzero(bg == 4)                                   # clone 3 absent from ALL of block 4; the cells 0 .. 9 have no counts there
    L[blk4, 3] = 0.0
    Y[:10][:, blk4] = 0
    E = mu[:, None] * L
    st, terms = host_terms(Y, E, U, V, bg, B, True)
    for k in ("within", "without", "between", "clone_loglik"):
        assert not np.isnan(terms[k]).any(), k
    check_terms(terms, Y, E, U, V, bg, B, True, f"zeros of E, D={D}")
    assert np.isneginf(terms["within"][7, 2, 1]) and np.isfinite(terms["within"][7, 2, [0, 2, 3, 4]]).all()
    assert np.isfinite(terms["without"][7, 2]).all()                 # (the offending gene is left out with its block) ...
    assert np.isfinite(terms["without"][:7, 4]).all() and np.isfinite(terms["without"][8:10, 4]).all()
    assert np.isneginf(terms["without"][7, [0, 1, 3, 4, 5], 1]).all()    # ... and stays in without any other block
    assert np.isneginf(st["logZ"][:, 4, 3]).all() and (st["A"][:10, 4, 3] == 0).all()
    assert (terms["within"][:10, 4] == 0).all()                      # E = 0 on all of the block against no counts: 0, not NaN
    busy = Y[:, blk4].sum(1) > 0
    assert np.isneginf(terms["within"][busy, 4, 3]).all() and np.isneginf(terms["clone_loglik"][busy, 3]).all()
    assert np.isfinite(terms["clone_loglik"][:10, 3][np.arange(10) != 7]).all()


def test_the_host_form_refuses_what_the_library_refuses():
    Y, L, mu, U, V, _rng = case_tables(40, 60, 3, 2, seed=3)
    E = mu[:, None] * L
    bg, B = interleaved_labels(60)
    for words, args in ((("n_blocks = 0",), (Y, E, U, V, bg, 0)), (("block_of_gene[4] = 4", "outside [0, 4)"), (Y, E, U, V, bg, 4)),
                        (("60 genes",), (Y, E, U, V, bg[:-1], B))):
        with pytest.raises(ValueError) as ex:
            api._clone_loglik_by_block_host(*args)
        assert all(w in str(ex.value) for w in words), str(ex.value)
    bad = U.copy()
    bad[9, 1] = np.nan
    with pytest.raises(ValueError, match="U has a non-finite entry"):
        api._clone_loglik_by_block_host(Y, E, bad, V, bg, B)
    Eb = E.copy()
    Eb[17, 2] = -1.0
    with pytest.raises(ValueError, match="gene 17, clone 2"):
        api._clone_loglik_by_block_host(Y, Eb, U, V, bg, B)


class HostOnly:                                                       # a live engine without device sums: the CPU host forms
    def __init__(self, N, G):
        self.N, self.G = N, G


def planted_fit(N, G, C, seed, K=1):
    rng = np.random.default_rng(seed)
    case = make_case(N=N, G=G, C=C, K=K, seed=seed, scale=1.0)       # planted clones
    alpha = rng.dirichlet(np.full(C, 5.0))
    fit = ca.ClonealignFit(ml_params={"mu": rng.lognormal(0, 1, G), "alpha": alpha, "W": rng.normal(size=(G, K)) * 0.2, "psi": rng.normal(size=(N, K))},
                           clone_names=[f"c{i}" for i in range(C)])
    return case["Y"], case["L"], fit, rng


def without_columns(fit, keep):
    ml = dict(fit["ml_params"])
    ml["mu"], ml["W"] = ml["mu"][keep], ml["W"][keep]
    return ca.ClonealignFit(ml_params=ml, clone_names=fit["clone_names"])


@pytest.mark.parametrize("psi", [None, "fit"])
def test_assignment_support_against_assign_cells_on_the_column_deleted_problems(psi):
    N, G, C = 400, 120, 3
    Y, L, fit, rng = planted_fit(N, G, C, seed=17)
    blocks = np.array(["chr1"] * 30 + ["chr2"] * 15 + ["chr7"] * 50 + ["chrX"] * 25, dtype=object)
    extra = rng.normal(size=(N, C))
    eng = HostOnly(N, G)
    sup = ca.assignment_support(fit, Y, L, blocks, extra_loglik=extra, psi=psi, engine=eng)
    ref = ca.assign_cells(fit, Y, L, extra_loglik=extra, psi=psi, engine=eng)
    for k in ("clone_probs", "loglik", "clone_loglik"):
        assert np.array_equal(sup[k], ref[k]), k
    assert np.array_equal(sup["clone"], ref["clone"]) and sup["clone_names"] == ref["clone_names"]
    assert list(sup["block_names"]) == ["chr1", "chr2", "chr7", "chrX"]
    B = 4
    assert sup["probs_without"].shape == (N, B, C) and sup["clone_without"].shape == (N, B) and sup["n_flips"].shape == (B,)
    cstar = ref["clone_probs"].argmax(1)
    t = ref["clone_loglik"] + np.log(fit["ml_params"]["alpha"])[None, :] + extra
    rest = np.where(np.arange(C)[None, :] == cstar[:, None], -np.inf, t)
    np.testing.assert_allclose(sup["margin"], t[np.arange(N), cstar] - rest.max(1), rtol=1e-12, atol=1e-9)
    assert (sup["margin"] >= 0).all()
    for b, name in enumerate(sup["block_names"]):
        keep = np.flatnonzero(blocks != name)
        sub = ca.assign_cells(without_columns(fit, keep), Y[:, keep], L[keep], extra_loglik=extra, psi=psi, engine=HostOnly(N, keep.size))
        assert np.abs(sup["probs_without"][:, b] - sub["clone_probs"]).max() <= 1e-9
        sure = np.abs(sub["clone_probs"].max(1) - 0.95) > 1e-6        # (a label can differ only where the maximum sits on the threshold)
        assert np.array_equal(sup["clone_without"][sure, b], sub["clone"][sure])
        flipped = sub["clone_probs"].argmax(1) != cstar
        assert sup["n_flips"][b] == int(flipped.sum())
        assert np.array_equal(sup["margin_without"][:, b] < 0, flipped)
        only = np.flatnonzero(blocks == name)
        alone = api._clone_loglik_host(Y[:, only], (fit["ml_params"]["mu"][:, None] * L)[only], None if psi is None else fit["ml_params"]["psi"],
                                       None if psi is None else fit["ml_params"]["W"][only])
        rest = np.where(np.arange(C)[None, :] == cstar[:, None], -np.inf, alone)
        np.testing.assert_allclose(sup["margin_within"][:, b], alone[np.arange(N), cstar] - rest.max(1), rtol=1e-9, atol=1e-8)
    assert sup["n_flips"].sum() > 0                                  # (the problem is small enough for some call to rest on one block)


def test_assignment_support_edges():
    N, G, C = 60, 40, 3
    Y, L, fit, _rng = planted_fit(N, G, C, seed=5)
    eng = HostOnly(N, G)
    one = ca.assignment_support(fit, Y, L, ["all"] * G, engine=eng)
    assert one["block_names"] == ["all"] and (one["without"] == 0).all() and np.allclose(one["probs_without"][:, 0], fit["ml_params"]["alpha"][None, :])
    by = ca.clone_loglik_by_block(fit, Y, L, ["all"] * G, engine=eng)
    assert (by["without"] == 0).all() and (by["between"] == 0).all() and np.array_equal(by["counts"][:, 0], Y.sum(1))
    labels = ["a", None, "b", float("nan")] * (G // 4)
    na = ca.clone_loglik_by_block(fit, Y, L, labels, engine=eng)
    assert na["block_names"] == ["a", "b", "NA"]
    assert np.array_equal(na["counts"][:, 2], Y[:, 1::2].sum(1))
    part = ca.clone_loglik_by_block(fit, Y, L, labels, engine=eng, cells=(10, 25))
    assert np.array_equal(part["within"], na["within"][10:25]) and np.array_equal(part["without"], na["without"][10:25])
    with pytest.raises(ValueError, match="C = 1"):
        ca.assignment_support(ca.ClonealignFit(ml_params={"mu": fit["ml_params"]["mu"]}), Y, L[:, :1], labels, engine=eng)
    with pytest.raises(ValueError, match="39 labels"):
        ca.clone_loglik_by_block(fit, Y, L, labels[:-1], engine=eng)
    # a cell that no clone can have produced: NaN margins, "unassigned"; a cell only one clone can have produced: +inf
    L0 = L.copy()
    L0[3, :] = 0.0
    L0[5, 1:] = 0.0
    Y0 = Y.copy()
    Y0[:, [3, 5]] = 0
    Y0[0, 3] = 1
    Y0[1, 5] = 1
    sup = ca.assignment_support(fit, Y0, L0, ["p"] * 20 + ["q"] * 20, engine=eng, saturate=False)
    assert np.isnan(sup["margin"][0]) and np.isnan(sup["margin_without"][0, 1]) and sup["clone"][0] == "unassigned"
    assert np.isfinite(sup["margin_without"][0, 0]) and sup["clone_without"][0, 1] == "unassigned"      # (the impossible count leaves with block p)
    assert np.isposinf(sup["margin"][1]) and np.isposinf(sup["margin_without"][1, 1]) and np.isfinite(sup["margin_without"][1, 0])
    assert np.isfinite(sup["margin"][2:]).all() and not np.isnan(sup["margin_without"][1:]).any()
