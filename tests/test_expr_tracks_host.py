"""plot_clonealign / clone_expression_profile (R/plotting.R:70-226): the host form, the track tables, the argument checks and the exported names.
No GPU needed: a stub engine without ``logexpr_sums`` sends every call through the chunked float64 host form."""
import os

import numpy as np
import pytest

import clonealign_amd
from clonealign_amd import api, engine
from clonealign_amd import plot_clonealign, clone_expression_profile   # fails on a tree without the feature

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class HostOnlyEngine:
    """A live engine without logexpr_sums: clone_expression_profile must take the host form."""

    def __init__(self, N, G):
        self.N, self.G = N, G


# 4 cells (A, A, B, C) x 6 genes, size factors 1, counts 0 or 15 so that lc = log2(y + 1) is 0 or 4.
#   a gene with lc = (4, 4, 4, 0) in some order: mean 3, deviations (1, 1, 1, -3), sd = sqrt(12 / 3) = 2, z = (.5, .5, .5, -1.5)
#   gene 2 has lc = (0, 0, 0, 4): mean 1, sd 2, z = (-.5, -.5, -.5, 1.5);  gene 5 is zero everywhere: sd 0 -> 1, z = 0
#                         low cell     mean z of  A      B      C
#   gene 0  (0, 15, 15, 15)   cell 0             -0.5    0.5    0.5
#   gene 1  (15, 15, 0, 15)   cell 2              0.5   -1.5    0.5
#   gene 2  (0, 0, 0, 15)     (high: cell 3)     -0.5   -0.5    1.5
#   gene 3  (15, 15, 0, 15)   cell 2              0.5   -1.5    0.5
#   gene 4  (15, 15, 15, 0)   cell 3              0.5    0.5   -1.5
#   gene 5  zeros                                 0      0      0
# positions (start + end) / 2 = 15, 30, 30, 60, 5, 110 -> ranks 2, 3.5, 3.5, 5, 1, 6 (genes 1 and 2 tie)
# in rank order (genes 4, 0, 1, 2, 3, 5) the copy-number rows are (2,2,2) (2,2,2) | (2,3,2) (2,3,2) (2,3,2) | (1,3,2): states 1 1 2 2 2 3
#   state 1 = genes 4, 0: ranks 1..2;   state 2 = genes 1, 2, 3: ranks 3.5..5;   state 3 = gene 5: rank 6
#   per (clone, state) mean of the genes' mean z:  A: (0, 1/6, 0)   B: (0.5, -7/6, 0)   C: (-0.5, 5/6, 0)
Y_HAND = np.array([[0, 15, 0, 15, 15, 0],
                   [15, 15, 0, 15, 15, 0],
                   [15, 0, 0, 0, 15, 0],
                   [15, 15, 15, 15, 0, 0]], dtype=np.int32)
CLONES_HAND = np.array(["A", "A", "B", "C"], dtype=object)
L_HAND = np.array([[2, 2, 2], [2, 3, 2], [2, 3, 2], [2, 3, 2], [2, 2, 2], [1, 3, 2]], dtype=np.float64)
START_HAND = np.array([10, 30, 30, 50, 5, 100])
END_HAND = np.array([20, 30, 30, 70, 5, 120])
MEAN_Z_HAND = np.array([[-0.5, 0.5, 0.5], [0.5, -1.5, 0.5], [-0.5, -0.5, 1.5], [0.5, -1.5, 0.5], [0.5, 0.5, -1.5], [0.0, 0.0, 0.0]])


class Frame:
    """The two attributes of a DataFrame that the package looks at."""

    def __init__(self, values, columns):
        self.values, self.columns = np.asarray(values), list(columns)


def hand_sce(Y=Y_HAND, **extra):
    row = {"chr": np.array(["1"] * Y.shape[1]), "start_position": START_HAND, "end_position": END_HAND}
    row.update(extra)
    return {"assays": {"counts": np.ascontiguousarray(Y.T)}, "rowData": row}


def hand_tracks(**kw):
    kw.setdefault("jitter_cnv", False)
    kw.setdefault("size_factors", np.ones(4))
    kw.setdefault("engine", HostOnlyEngine(4, 6))
    return plot_clonealign(hand_sce(), kw.pop("clones", CLONES_HAND), Frame(L_HAND, "ABC"), **kw)


def test_profile_of_the_case_worked_by_hand():
    prof = clone_expression_profile(Y_HAND, CLONES_HAND, size_factors=np.ones(4), engine=HostOnlyEngine(4, 6))
    assert prof["labels"] == ["A", "B", "C"] and prof["n_cells"].tolist() == [2, 1, 1]
    np.testing.assert_allclose(prof["mean"], [3, 3, 1, 3, 3, 0], rtol=1e-15)
    np.testing.assert_allclose(prof["sd"], [2, 2, 2, 2, 2, 1], rtol=1e-15)       # the all-zero gene: sd 0 -> 1
    np.testing.assert_allclose(prof["mean_z"], MEAN_Z_HAND, rtol=1e-15, atol=0)
    assert np.all(prof["mean_z"][5] == 0.0)                                       # ... and z exactly 0


def test_tracks_of_the_case_worked_by_hand():
    t = hand_tracks()
    assert isinstance(t, clonealign_amd.ClonealignTracks) and t.genes is t["genes"]
    np.testing.assert_array_equal(t.genes["rank_position"], [2, 3.5, 3.5, 5, 1, 6])
    np.testing.assert_array_equal(t.genes["state"], [1, 2, 2, 2, 1, 3])
    np.testing.assert_array_equal(t.genes["ensembl_gene_id"], ["1", "2", "3", "4", "5", "6"])
    cs = t.cnv_segments
    np.testing.assert_array_equal(cs["state"], [1, 1, 1, 2, 2, 2, 3, 3, 3])
    np.testing.assert_array_equal(cs["clone"], list("ABC") * 3)
    np.testing.assert_array_equal(cs["copy_number"], [2, 2, 2, 2, 3, 2, 1, 3, 2])     # exact without jitter
    np.testing.assert_array_equal(cs["start"], [1, 1, 1, 3.5, 3.5, 3.5, 6, 6, 6])
    np.testing.assert_array_equal(cs["end"], [2, 2, 2, 5, 5, 5, 6, 6, 6])
    np.testing.assert_array_equal(cs["length"], [1, 1, 1, 1.5, 1.5, 1.5, 0, 0, 0])
    ex = t.expression
    np.testing.assert_array_equal(ex["clone"], np.repeat(list("ABC"), 6))
    np.testing.assert_array_equal(ex["gene_index"], np.tile(np.arange(6), 3))
    np.testing.assert_allclose(ex["mean_z_score"], MEAN_Z_HAND.T.reshape(-1), rtol=1e-15)
    es = t.expression_segments
    np.testing.assert_array_equal(es["state"], cs["state"])
    np.testing.assert_array_equal(es["clone"], cs["clone"])
    np.testing.assert_array_equal(es["start"], cs["start"])
    np.testing.assert_array_equal(es["end"], cs["end"])
    np.testing.assert_allclose(es["per_clone_state_z_score"], [0, 0.5, -0.5, 1 / 6, -7 / 6, 5 / 6, 0, 0, 0], rtol=1e-15, atol=1e-16)


def test_genes_of_other_chromosomes_are_left_out_and_ids_are_kept():
    Y = np.concatenate([Y_HAND, np.array([[3], [0], [1], [7]], dtype=np.int32)], axis=1)
    row = {"chr": np.array(["1"] * 6 + ["X"]), "start_position": np.r_[START_HAND, 1], "end_position": np.r_[END_HAND, 2],
           "ensembl_gene_id": np.array([f"ENSG{i}" for i in range(7)])}
    sce = {"assays": {"counts": np.ascontiguousarray(Y.T)}, "rowData": row}
    L = np.concatenate([L_HAND, [[4, 4, 4]]])
    t = plot_clonealign(sce, CLONES_HAND, Frame(L, "ABC"), jitter_cnv=False, size_factors=np.ones(4), engine=HostOnlyEngine(4, 7))
    np.testing.assert_array_equal(t.genes["gene_index"], np.arange(6))
    np.testing.assert_array_equal(t.genes["ensembl_gene_id"], [f"ENSG{i}" for i in range(6)])
    np.testing.assert_array_equal(t.genes["state"], [1, 2, 2, 2, 1, 3])
    np.testing.assert_allclose(t.expression["mean_z_score"], MEAN_Z_HAND.T.reshape(-1), rtol=1e-15)
    x = plot_clonealign(sce, CLONES_HAND, Frame(L, "ABC"), chromosome="X", jitter_cnv=False, profile=t.profile)    # a second chromosome: no new sweep
    assert x.genes["gene_index"].tolist() == [6] and x.genes["state"].tolist() == [1] and x.cnv_segments["length"].tolist() == [0, 0, 0]


def test_jitter_is_off_exact_and_reproducible_under_a_seed():
    plain = hand_tracks(jitter_cnv=False)
    a, b, c = hand_tracks(jitter_cnv=True, seed=5), hand_tracks(jitter_cnv=True, seed=5), hand_tracks(jitter_cnv=True, seed=6)
    np.testing.assert_array_equal(a.cnv_segments["copy_number"], b.cnv_segments["copy_number"])
    assert not np.array_equal(a.cnv_segments["copy_number"], c.cnv_segments["copy_number"])
    d = a.cnv_segments["copy_number"] - plain.cnv_segments["copy_number"]
    assert np.all(d != 0) and np.abs(d).max() < 0.1 * 6                            # N(0, 0.1) noise on every segment
    np.testing.assert_array_equal(a.expression_segments["copy_number"], a.cnv_segments["copy_number"])
    wide = hand_tracks(jitter_cnv=True, seed=5, cnv_dodge_sd=1.0)
    np.testing.assert_allclose(wide.cnv_segments["copy_number"] - plain.cnv_segments["copy_number"], 10 * d, rtol=1e-12)
    np.testing.assert_array_equal(a.cnv_segments["start"], plain.cnv_segments["start"])


def test_the_four_error_messages_of_the_reference():
    cnv = Frame(L_HAND, "ABC")
    eng = HostOnlyEngine(4, 6)
    with pytest.raises(ValueError) as ex:
        plot_clonealign(hand_sce(), CLONES_HAND, cnv, chr_str="chromosome", engine=eng)
    assert str(ex.value) == "The column 'chr_str' (currently set to 'chromosome') must be in rowData(sce) and refer to the chromosome of each gene"
    with pytest.raises(ValueError) as ex:
        plot_clonealign(hand_sce(), CLONES_HAND, cnv, start_str="start_pos", engine=eng)
    assert str(ex.value) == "The column 'start_str' (currently set to 'start_pos') must be in rowData(sce) and refer to the start position of each gene"
    with pytest.raises(ValueError) as ex:
        plot_clonealign(hand_sce(), CLONES_HAND, cnv, end_str="end_pos", engine=eng)
    assert str(ex.value) == "The column 'end_str' (currently set to 'end_pos') must be in rowData(sce) and refer to the end position of each gene"
    with pytest.raises(ValueError) as ex:
        plot_clonealign(hand_sce(), CLONES_HAND, cnv, chromosome="7", engine=eng)
    assert str(ex.value) == "No genes on chromosome 7 in CNV regions"


def test_unassigned_cells_are_a_label_of_the_expression_but_have_no_segments():
    clones = np.array(["A", "unassigned", "B", "C"], dtype=object)
    t = hand_tracks(clones=clones)
    assert t.labels == ["A", "unassigned", "B", "C"]
    assert "unassigned" in set(t.expression["clone"]) and (t.expression["clone"] == "unassigned").sum() == 6
    assert set(t.expression_segments["clone"]) == {"A", "B", "C"} and set(t.cnv_segments["clone"]) == {"A", "B", "C"}
    # the unassigned cell is cell 1: its own z-scores per gene (one cell: the mean is the value)
    np.testing.assert_allclose(t.expression["mean_z_score"][t.expression["clone"] == "unassigned"], [0.5, 0.5, -0.5, 0.5, 0.5, 0.0], rtol=1e-15)


def test_host_form_default_size_factors_chunks_and_sparse_input():
    import scipy.sparse as sps
    rng = np.random.default_rng(4)
    N, G, Q = 61, 17, 4
    Y = rng.poisson(1.2, size=(N, G)).astype(np.int32)
    Y[:, 0] += 1
    Y[:, 3] = 0
    idx = rng.integers(-1, Q, N)
    used = idx >= 0
    lib = Y.sum(1).astype(np.float64)
    sf = lib / lib[used].mean()                                       # centred at 1 over the USED cells
    lc = np.log2(Y / sf[:, None] + 1.0)
    a = api._logexpr_sums_host(Y, idx, Q)
    b = api._logexpr_sums_host(sps.csr_matrix(Y), idx, Q, chunk=7)
    for out in (a, b):
        assert out["n_group"].tolist() == np.bincount(idx[used], minlength=Q).tolist()
        np.testing.assert_allclose(out["S2"], (lc[used] ** 2).sum(0), rtol=1e-13)
        for q in range(Q):
            np.testing.assert_allclose(out["S1"][:, q], lc[idx == q].sum(0), rtol=1e-13)
    # the profile against the plain two-pass form over all cells
    clones = np.array(["c%d" % i for i in rng.integers(0, Q, N)], dtype=object)
    prof = clone_expression_profile(Y, clones, engine=HostOnlyEngine(N, G))
    lc = np.log2(Y / (lib / lib.mean())[:, None] + 1.0)
    sd = lc.std(0, ddof=1)
    sd[sd == 0] = 1
    np.testing.assert_allclose(prof["mean"], lc.mean(0), rtol=1e-13)
    np.testing.assert_allclose(prof["sd"], sd, rtol=1e-12)
    assert prof["sd"][3] == 1.0 and np.all(prof["mean_z"][3] == 0.0)
    for q, lab in enumerate(prof["labels"]):
        np.testing.assert_allclose(prof["mean_z"][:, q], ((lc - lc.mean(0)) / sd)[clones == lab].mean(0), rtol=1e-10, atol=1e-13)


def test_host_form_refuses_what_the_device_pass_refuses():
    Y = np.ones((5, 3), dtype=np.int32)
    with pytest.raises(ValueError, match=r"n_groups = 65"):
        api._logexpr_sums_host(Y, np.zeros(5, dtype=int), 65)
    with pytest.raises(ValueError, match=r"group index 2 of cell 4"):
        api._logexpr_sums_host(Y, [0, 1, 0, -1, 2], 2)
    Y[2] = 0
    with pytest.raises(ValueError, match=r"cell 2 .*size factor"):
        api._logexpr_sums_host(Y, [0, 1, 0, -1, 1], 2)
    assert api._logexpr_sums_host(Y, [0, 1, -1, -1, 1], 2)["n_group"].tolist() == [1, 2]      # the empty cell left out: fine
    with pytest.raises(ValueError, match="labels"):
        clone_expression_profile(Y, ["A"] * 4, engine=HostOnlyEngine(5, 3))
    with pytest.raises(ValueError, match="engine holds"):
        class Eng(HostOnlyEngine):
            def logexpr_sums(self, *a):
                raise AssertionError("not reached")
        clone_expression_profile(Y, ["A"] * 5, engine=Eng(6, 3))


def test_example_fixture_with_the_vignette_positions():
    """R/plotting.R:52-62: genes placed in the order of their sorted copy-number rows, so each distinct row is one contiguous state."""
    d = np.load(os.path.join(GOLDEN, "example_sce.npz"))
    Y, L = d["Y"], d["L"]
    N, G = Y.shape
    order = np.lexsort((L[:, 2], L[:, 1], L[:, 0]))                  # arrange(A, B, C)
    position = np.empty(G, dtype=np.int64)
    position[order] = np.arange(1, G + 1)
    sce = {"assays": {"counts": np.ascontiguousarray(Y.T)}, "rownames": list(d["genes"]),
           "rowData": {"chromosome": np.array(["1"] * G), "start_pos": position, "end_pos": position}}
    clones = np.random.default_rng(0).choice(np.array(["A", "B", "C", "unassigned"], dtype=object), size=N)
    t = plot_clonealign(sce, clones, Frame(L, [str(c) for c in d["clones"]]), chromosome="1", chr_str="chromosome", start_str="start_pos",
                        end_str="end_pos", seed=1, engine=HostOnlyEngine(N, G))
    n_rows = len(np.unique(L, axis=0))
    assert t.genes["state"].max() == n_rows and len(np.unique(t.genes["state"])) == n_rows
    np.testing.assert_array_equal(t.genes["rank_position"], position)
    for st in range(1, n_rows + 1):                                  # a state holds exactly the genes of one copy-number row
        assert len(np.unique(L[t.genes["state"] == st], axis=0)) == 1
    cs = t.cnv_segments
    assert len(cs["state"]) == 3 * n_rows
    for c in "ABC":
        assert (cs["length"][cs["clone"] == c] + 1).sum() == G       # the segments tile the chromosome
    assert np.all(np.abs(cs["copy_number"] - np.round(cs["copy_number"])) < 0.6) and not np.all(cs["copy_number"] == np.round(cs["copy_number"]))
    assert len(t.expression["mean_z_score"]) == 4 * G and np.all(np.isfinite(t.expression["mean_z_score"]))
    assert set(t.expression_segments["clone"]) == {"A", "B", "C"}
    # z-scores of all cells average to zero per gene: sum over labels of n_q * mean_z = 0
    np.testing.assert_allclose(t.profile["mean_z"] @ t.profile["n_cells"], 0, atol=1e-9)


def test_draw_without_matplotlib_says_that_the_tracks_are_the_result():
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="tracks themselves"):
            hand_tracks().draw()
    else:
        import matplotlib
        matplotlib.use("Agg")
        assert hand_tracks().draw() is not None


def test_new_names_are_exported():
    assert "ca_logexpr_sums" in engine.EXPORTS and "ca_group_logexpr_sums" in engine.EXPORTS
    assert callable(engine.HipEngine.logexpr_sums) and engine.HipGroupEngine.logexpr_sums is engine.HipEngine.logexpr_sums
    assert clonealign_amd.plot_clonealign is api.plot_clonealign and clonealign_amd.clone_expression_profile is api.clone_expression_profile
