"""The inputs of tests/test_gpu_device_helpers.py meet their own conditions (numpy only, no device): the storage each variant is meant to
land in, the eigenvalue gaps and column spreads that make the PCA comparison well posed, and large-count totals on which a rounded float32
partial sum cannot hide."""
import numpy as np
import pytest

from tests import _device_helper_cases as dc


@pytest.mark.parametrize("shape", dc.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", dc.VARIANTS)
def test_variant_lands_in_its_storage_and_pca_is_well_posed(kind, shape):
    Y = dc.variant(kind, *shape)
    assert Y.shape == shape and Y.min() >= 0 and (Y.sum(0) > 0).all() and (Y.sum(1) > 0).all()
    store, n_ovf = dc.auto_storage(Y)
    if dc.storage_arg(kind, Y) == "auto":
        assert store == dc.STORAGE[kind]
    else:   # the one forced storage: f32int where the shape's counts stay below 65536
        assert kind == "f32int" and store == "u16" and Y.max() < 65536
    assert (n_ovf > 0) == (kind == "u8ovf")
    if kind == "f32int":
        assert Y.max() < (1 << 24) and np.array_equal(Y, Y.astype(np.float32))
    if kind == "f32frac":
        assert np.array_equal(Y * 2, np.floor(Y * 2)) and (Y != np.floor(Y)).sum() == Y.size // 50
    gap, sd = dc.pca_conditions(Y, 2)
    print(f"{kind} {shape}: min eigenvalue ratio {gap:.3f}, min column sd {sd:.3f}")
    assert gap >= dc.GAP_MIN, gap
    assert sd > dc.SD_MIN, sd


def test_f32int_is_forced_only_where_the_issue_says():
    forced = [s for s in dc.SHAPES if dc.storage_arg("f32int", dc.variant("f32int", *s)) != "auto"]
    assert (1100, 40) in forced or not forced
    for kind in ("u8", "u8ovf", "u16", "f32frac"):
        for s in dc.SHAPES:
            assert dc.storage_arg(kind, dc.variant(kind, *s)) == "auto", (kind, s)


def test_pca_model_error_is_a_float32_sized_number():
    for kind, shape in (("u8", (333, 95)), ("f32int", (257, 1030))):
        m = dc.pca_model_error(dc.variant(kind, *shape), 2)
        assert m.shape == (2,) and (m > 1e-8).all() and (m < 2e-5).all(), m


@pytest.mark.parametrize("labels", dc.LABELS)
@pytest.mark.parametrize("kind", dc.LARGE)
def test_large_count_totals_make_a_rounded_partial_sum_visible(kind, labels):
    N, G, C = dc.LARGE_SHAPE
    Y = dc.large_counts(kind)
    idx = dc.clone_labels(N, C, skew=labels == "skew")
    assert Y.shape == (N, G) and set(np.unique(idx)) == set(range(-1, C))
    assert dc.auto_storage(Y)[0] == dc.STORAGE[kind]
    if kind == "u8ovf":
        assert dc.auto_storage(Y)[1] == N        # one gene in every cell: 1/70 of the entries
    Yi = Y.astype(np.int64)
    T = np.stack([Yi[idx == c].sum(0) for c in range(C)], 1)
    assert T.max() < (1 << 53)
    assert (T % 2 == 1).mean() >= 0.25
    if kind == "u16" and labels == "uniform":
        # a fifth of 1100 cells per clone: no total of 16-bit counts can reach 2^24 (which is why the skewed labels exist); its float32 sum of y^2 can
        assert (idx == 0).sum() * 65535 < (1 << 24) < (Y[idx == 0] ** 2).sum(0).min()
    else:
        assert (T > (1 << 24)).any()
    Tref, Syy = dc.clone_sums_ref(Y, idx, C)
    assert np.array_equal(Tref, T.astype(np.float64)) and np.array_equal(Tref.astype(np.int64), T)
    assert (Y[idx >= 0].mean(0) >= 1e4).any()    # a gene whose n Syy - Sy^2 cancels
    r = dc.host_correlations(Y, dc.copy_numbers(G, C), idx)
    assert np.isfinite(r).all()


def test_readback_cells_cover_the_boundaries():
    Y = dc.variant("u8ovf", 700, 300)
    a, b = dc.readback_cells(Y, 4)
    cells = a + b
    assert len(set(cells)) == 8 and {0, 699, 127, 128, 255, 256}.issubset(cells)
    assert (Y[cells].max(1) > 255).any()
    idx = dc.one_cell_labels(700, a)
    assert [int(np.flatnonzero(idx == c)[0]) for c in range(4)] == a and (idx >= 0).sum() == 4


def test_preprocess_case_holds_f32int_sized_counts_exactly_in_float32():
    Y, L = dc.preprocess_case()
    assert Y.shape == (2500, 420) and 65535 < Y.max() < (1 << 24)
    assert np.array_equal(Y.astype(np.float32).astype(np.int64), Y)
    assert Y.sum(0).max() > (1 << 24) and Y.sum(1).max() > (1 << 24)      # sums a float32 accumulator would round
