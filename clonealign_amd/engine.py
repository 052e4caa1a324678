"""ctypes binding of ``libclonealign_hip.so`` (C ABI: ``include/clonealign_hip.h``).

This is the product path: there is NO CPU fallback.  Importing works anywhere (so the
symbol table can be checked without a GPU); constructing a :class:`HipEngine` fails loudly
when the library is missing or no MI355X is visible.
"""
import ctypes as C
import os

import numpy as np

from . import hostprep

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libclonealign_hip.so")

CA_OK = 0
CA_ERR_NAN = 4
CA_INTERRUPTED = 7
CA_ABI_VERSION = 6
P2P_HANDLE_BYTES = 128
CA_F64, CA_F32, CA_I32, CA_U16, CA_U8 = 0, 1, 2, 3, 4
CA_ROW_MAJOR, CA_COL_MAJOR = 0, 1
YSTORE = {"auto": 0, "f32": 1, "u16": 2, "u8": 3}
YSTORE_NAME = {v: k for k, v in YSTORE.items()}
KERNEL_NAMES = ("fwd", "bwd", "ypass", "cell", "other")
# ca_variant bits (ca_options.variant_off: a set bit switches the variant OFF) and ca_tune_id slots
VARIANTS = {"fused": 1 << 0, "fwd_mfma": 1 << 1, "fwd_cell": 1 << 2, "bwd_mfma": 1 << 3, "tail_fuse": 1 << 4, "async_y": 1 << 5,
            "pre": 1 << 6, "pair_elbo": 1 << 7, "prep_fast": 1 << 8, "update_merge": 1 << 9, "p2p": 1 << 10, "fold_gsum": 1 << 11, "y_ride": 1 << 12, "ride_seq": 1 << 13, "y_mfma1": 1 << 14, "yfin_ride": 1 << 15, "p2p_ride": 1 << 16, "run_gate": 1 << 17, "s2_fuse": 1 << 18, "fwd_bal": 1 << 19, "bwd_tl3": 1 << 20, "series": 1 << 21, "y4": 1 << 22, "mom_ride": 1 << 23, "cell_lean": 1 << 24, "mom_last": 1 << 25, "cell_mfma": 1 << 26, "y2": 1 << 27, "gene_ride": 1 << 28, "cell_edge": 1 << 29}
VARIANTS_ON = {"y_mfma2": 1 << 0, "async_small": 1 << 1, "y_mfma1": 1 << 2, "fold_always": 1 << 3, "ride_seq": 1 << 4, "p2p_same_device": 1 << 5, "run_fwd": 1 << 6, "bal_tiles": 1 << 7, "series": 1 << 8, "y4": 1 << 9, "mom_last": 1 << 10, "y2": 1 << 11}      # ca_variant_on: opt-in variants
OPT_VERBOSE = 0x80000000
TUNE = {"gsplit": 0, "fsplit": 1, "fc_tl": 2, "fc_nbig": 3, "csplit": 4, "csplit_m": 5, "tr": 6, "rg": 7}
TRANSPORT_NAME = {0: "none", 1: "rccl", 2: "host", 3: "p2p"}

EXPORTS = (
    "ca_abi_version", "ca_build_id", "ca_device_count", "ca_default_options", "ca_create", "ca_destroy", "ca_last_error", "ca_get_info",
    "ca_synchronize", "ca_stream_busy", "ca_comm_unique_id", "ca_comm_init", "ca_p2p_export", "ca_p2p_connect", "ca_p2p_commit", "ca_comm_benchmark", "ca_comm_selftest", "ca_set_host_allreduce", "ca_gamma_init", "ca_elbo", "ca_elbo_terms",
    "ca_step", "ca_gradients", "ca_run", "ca_run_ex", "ca_iterate", "ca_final_elbo", "ca_init_psi_pca", "ca_clone_gene_sums", "ca_get_param", "ca_set_param",
    "ca_get_gradient", "ca_reinit", "ca_get_kernel_times", "ca_reset_kernel_times", "ca_set_profile", "ca_eps_draw", "ca_allele_loglik", "ca_preprocess",
    # ABI 6: one fit cell-sharded over several devices of one process
    "ca_group_create", "ca_group_destroy", "ca_group_last_error", "ca_group_get_info", "ca_group_rank_handle", "ca_group_init_psi_pca", "ca_group_gamma_init",
    "ca_group_elbo", "ca_group_step", "ca_group_run_ex", "ca_group_iterate", "ca_group_final_elbo", "ca_group_get_param", "ca_group_reinit",
    "ca_group_clone_gene_sums",
    # sparse (CSR / CSC) count matrices, additions to ABI 6
    "ca_create_sparse", "ca_group_create_sparse",
    # squared error of a fit on the resident matrix (compute_ca_fit_mse), additions to ABI 6
    "ca_fit_mse", "ca_group_fit_mse",
    # log-expression sums per gene and cell group on the resident matrix (plot_clonealign), additions to ABI 6
    "ca_logexpr_sums", "ca_group_logexpr_sums",
    # per-cell, per-clone log-likelihood of the resident matrix under a fitted model (clone_loglik / assign_cells), additions to ABI 6
    "ca_clone_loglik", "ca_group_clone_loglik",
    # per-cell MAP psi and clone posterior of cells outside the fit (project_cells), additions to ABI 6
    "ca_project_cells", "ca_group_project_cells",
    # log-likelihood under every mixture of two clones on a weight grid (clone_pair_loglik / detect_doublets), additions to ABI 6
    "ca_clone_pair_loglik", "ca_group_clone_pair_loglik",
    # maximum-likelihood mixture of all clones per cell: simplex weights by projected Newton with a certified bound (clone_mixture / mixture_loglik /
    # deconvolve_clones), additions to ABI 6
    "ca_clone_mixture", "ca_group_clone_mixture",
    # Dirichlet-multinomial log-likelihood per clone on a grid of concentrations (clone_loglik_dm / estimate_concentration / assign_cells_dm), additions to ABI 6
    "ca_clone_loglik_dm", "ca_group_clone_loglik_dm",
    # the log-likelihood's sufficient statistics by block of genes (clone_loglik_by_block / assignment_support), additions to ABI 6
    "ca_clone_loglik_by_block", "ca_group_clone_loglik_by_block",
    # count rows drawn from a fitted model (simulate_counts), no handle, additions to ABI 6
    "ca_simulate_counts", "ca_simulate_kernel_ms",
    # log-likelihoods and per-clone gene totals of replicate rows that never leave the device (predictive_stats), no handle, additions to ABI 6
    "ca_predictive_stats", "ca_predictive_kernel_ms",
    # the replicates' moments in closed form: per cell the mean and variance of the log-likelihood's linear part, per (gene, clone) three cumulants of the totals
    # (predictive_moments), no handle, additions to ABI 6
    "ca_predictive_moments", "ca_predictive_moments_kernel_ms",
    # clone separability in closed form: per cell and ordered pair of clones the per-read moments of the log-likelihood ratio and the probability of an
    # excluding read (clone_separability / reads_needed / merge_candidates), no handle, additions to ABI 6
    "ca_clone_separability", "ca_clone_separability_kernel_ms",
    # the expression side of the likelihood profile over the copy-number matrix: per (gene or block of genes, clone, candidate copy number) the change of the
    # cells' normalisers (copy_number_profile / suspect_copy_numbers / apply_copy_number_calls), no handle, additions to ABI 6
    "ca_copy_number_profile", "ca_copy_number_profile_kernel_ms",
    # clone evidence with psi integrated out: Newton mode, Laplace value and quadrature per (cell, clone) (clone_evidence / heldout_evidence), additions to ABI 6
    "ca_clone_evidence", "ca_group_clone_evidence",
    # gene-reweighted log-likelihood for every replicate of a bootstrap, votes and shares reduced on the device (clone_loglik_reweighted / bootstrap_assignments),
    # additions to ABI 6
    "ca_clone_loglik_reweighted", "ca_group_clone_loglik_reweighted", "ca_reweighted_kernel_ms",
    # the count-matrix stream's partial slabs, exponents and fixed-point images, read-only (ystream_parts), addition to ABI 6
    "ca_ystream_parts",
)
CA_BOOT_RCHUNK = 32   # replicates per chunk of ca_clone_loglik_reweighted (include/clonealign_hip.h)


def reweighted_cells_per_batch(n, G, C, D, R):
    """Cells per internal batch of ``clone_loglik_reweighted`` on ``n`` cells: the library's arithmetic (ca_clone_loglik_reweighted in
    csrc/ca_eng_score.inc: the slabs of a batch stay below a quarter of a gigabyte, whole blocks of 256 cells), restated so that a test can tell whether a
    call spans two batches.  No result depends on it."""
    rc = min(int(R), CA_BOOT_RCHUNK)
    nzc, nw = -(-int(G) // 512), -(-int(C) // 32)
    nc1, nc2 = -(-rc * (C + 1) // 16) * 16, -(-rc * C // 16) * 16
    per_cell = (nzc * (nc1 + (nc2 + 1 if D > 0 else 0)) + rc * (C + 1) + 2 * C) * 8 + (rc * nw + C) * 4
    return min(int(n), max(256, ((1 << 28) // per_cell) // 256 * 256))
CA_SPARSE_CSR, CA_SPARSE_CSC = 0, 1


class CaProblem(C.Structure):
    _fields_ = [("N", C.c_int64), ("G", C.c_int32), ("C", C.c_int32), ("K", C.c_int32), ("P", C.c_int32),
                ("S", C.c_int32), ("layout", C.c_int32), ("y_dtype", C.c_int32), ("y_on_device", C.c_int32),
                ("Y", C.c_void_p), ("L", C.c_void_p), ("psi0", C.c_void_p), ("loc0", C.c_void_p),
                ("X", C.c_void_p), ("extra_loglik", C.c_void_p),
                ("N_src", C.c_int64), ("G_src", C.c_int32), ("cell_index", C.c_void_p), ("gene_index", C.c_void_p),
                ("y_ld", C.c_int64)]


class CaSparse(C.Structure):
    _fields_ = [("kind", C.c_int32), ("val_dtype", C.c_int32), ("index_bytes", C.c_int32), ("on_device", C.c_int32),
                ("nnz", C.c_int64), ("ptr", C.c_void_p), ("idx", C.c_void_p), ("val", C.c_void_p)]


class CaOptions(C.Structure):
    _fields_ = [("learning_rate", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double),
                ("adam_eps", C.c_double), ("seed", C.c_uint64), ("device", C.c_int32),
                ("y_storage", C.c_int32), ("rank", C.c_int32), ("world", C.c_int32), ("profile", C.c_int32),
                ("variant_off", C.c_uint32), ("tune", C.c_int32 * 8), ("variant_on", C.c_uint32),
                ("ride_pattern", C.c_int32), ("comm_timeout_ms", C.c_int32), ("gate_timeout_us", C.c_int32), ("reserved", C.c_int32 * 2)]


class CaInfo(C.Structure):
    _fields_ = [("N", C.c_int64), ("G", C.c_int32), ("C", C.c_int32), ("K", C.c_int32), ("P", C.c_int32),
                ("S", C.c_int32), ("y_storage", C.c_int32), ("y_bytes_per_elem", C.c_int32),
                ("y_device_bytes", C.c_int64), ("device_bytes", C.c_int64), ("gsplit", C.c_int32),
                ("csplit", C.c_int32), ("n_cu", C.c_int32), ("fused_sweep", C.c_int32), ("fwd_mfma", C.c_int32),
                ("bwd_mfma", C.c_int32), ("fsplit", C.c_int32), ("fwd_cell", C.c_int32), ("y_mfma", C.c_int32),
                ("transport", C.c_int32), ("y_ride", C.c_int32), ("red_n", C.c_int64),
                ("fwd_block_cells", C.c_int32), ("fwd_blocks_big", C.c_int32), ("fold_gsum", C.c_int32), ("yfin_split", C.c_int32),
                ("update_merge", C.c_int32), ("fwd_balanced", C.c_int32), ("fwd_series", C.c_int32), ("y_stream_bits", C.c_int32),
                ("series_passes", C.c_int64), ("series_fallbacks", C.c_int64), ("mom_ride", C.c_int32), ("cell_lean", C.c_int32),
                ("mom_last", C.c_int32), ("mom_free_slots", C.c_int32), ("cell_mfma", C.c_int32),
                ("y_stream_n2", C.c_int32), ("y_stream_esc", C.c_int64), ("y_stream_bytes", C.c_int64), ("gene_ride", C.c_int32),
                ("cell_edge", C.c_int32)]


class CaGroupInfo(C.Structure):
    _fields_ = [("world", C.c_int32), ("transport", C.c_int32), ("p2p_status", C.c_int32), ("rccl_status", C.c_int32),
                ("rebuilds", C.c_int32), ("selftest_rounds", C.c_int32), ("N", C.c_int64), ("note", C.c_char * 384)]


class CaPreprocessParams(C.Structure):
    _fields_ = [("min_counts_per_gene", C.c_double), ("min_counts_per_cell", C.c_double),
                ("remove_outlying_genes", C.c_int32), ("remove_genes_same_copy_number", C.c_int32),
                ("nmads", C.c_double), ("max_copy_number", C.c_double)]


HOST_ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int64)
POLL_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.c_double)

_lib = None


def _ptr(a, empty_null=False):
    """The C pointer of array ``a``; NULL for None and, when asked, for an array without elements."""
    return None if a is None or (empty_null and a.size == 0) else a.ctypes.data_as(C.c_void_p)


def load_library(path=None):
    """dlopen the engine; raises (never falls back) when it is not built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("CLONEALIGN_HIP_LIB") or LIB_PATH     # (the override is for A/B builds of the same ABI)
    if not os.path.exists(p):
        raise RuntimeError(
            f"{p} not found: build the HIP engine first (python -c 'import __graft_entry__ as g; g.build()' "
            "or make -C clonealign_amd/csrc). clonealign_amd has no CPU fallback.")
    lib = C.CDLL(p)
    lib.ca_last_error.restype = C.c_char_p
    lib.ca_last_error.argtypes = [C.c_void_p]
    lib.ca_build_id.restype = C.c_char_p
    lib.ca_build_id.argtypes = []
    lib.ca_group_last_error.restype = C.c_char_p
    lib.ca_group_last_error.argtypes = [C.c_void_p]
    for name in EXPORTS:
        if name not in ("ca_last_error", "ca_build_id", "ca_group_last_error"):
            getattr(lib, name).restype = C.c_int
    lib.ca_device_count.argtypes = [C.POINTER(C.c_int32)]
    lib.ca_create.argtypes = [C.POINTER(CaProblem), C.POINTER(CaOptions), C.POINTER(C.c_void_p)]
    lib.ca_create_sparse.argtypes = [C.POINTER(CaProblem), C.POINTER(CaSparse), C.POINTER(CaOptions), C.POINTER(C.c_void_p)]
    lib.ca_destroy.argtypes = [C.c_void_p]
    lib.ca_get_info.argtypes = [C.c_void_p, C.POINTER(CaInfo)]
    lib.ca_synchronize.argtypes = [C.c_void_p]
    lib.ca_stream_busy.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    lib.ca_ystream_parts.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ca_comm_unique_id.argtypes = [C.c_char_p]
    lib.ca_comm_init.argtypes = [C.c_void_p, C.c_char_p]
    lib.ca_p2p_export.argtypes = [C.c_void_p, C.c_char_p]
    lib.ca_p2p_connect.argtypes = [C.c_void_p, C.c_char_p]
    lib.ca_p2p_commit.argtypes = [C.c_void_p, C.c_int32]
    lib.ca_comm_benchmark.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_double)]
    lib.ca_comm_selftest.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.POINTER(C.c_int64)]
    lib.ca_set_host_allreduce.argtypes = [C.c_void_p, HOST_ALLREDUCE_FN, C.c_void_p]
    lib.ca_gamma_init.argtypes = [C.c_void_p, C.c_void_p]
    lib.ca_elbo.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
    lib.ca_elbo_terms.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
    lib.ca_step.argtypes = [C.c_void_p, C.c_void_p]
    lib.ca_gradients.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
    lib.ca_run.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_int64, C.c_void_p,
                           C.POINTER(C.c_int32)]
    lib.ca_run_ex.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_int64, C.c_void_p,
                              C.POINTER(C.c_int32), POLL_FN, C.c_void_p]
    lib.ca_iterate.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_double)]
    lib.ca_final_elbo.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                                  C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.ca_init_psi_pca.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p]
    lib.ca_clone_gene_sums.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ca_fit_mse.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_void_p, C.c_void_p]
    lib.ca_logexpr_sums.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ca_clone_loglik.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.ca_clone_pair_loglik.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_int64,
                                         C.c_void_p, C.c_void_p]
    lib.ca_clone_loglik_dm.argtypes = lib.ca_clone_pair_loglik.argtypes
    lib.ca_clone_mixture.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_double, C.c_int64, C.c_int64,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ca_clone_loglik_by_block.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_int64,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ca_project_cells.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                     C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ca_clone_evidence.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                      C.c_int32, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ca_simulate_counts.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64,
                                       C.c_int64, C.c_int32, C.c_void_p, C.c_char_p]
    lib.ca_simulate_kernel_ms.argtypes = [C.POINTER(C.c_double)]
    lib.ca_predictive_stats.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64,
                                        C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_char_p]
    lib.ca_predictive_kernel_ms.argtypes = [C.POINTER(C.c_double)]
    lib.ca_predictive_moments.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p]
    lib.ca_predictive_moments_kernel_ms.argtypes = [C.POINTER(C.c_double)]
    lib.ca_clone_separability.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p]
    lib.ca_clone_separability_kernel_ms.argtypes = [C.POINTER(C.c_double)]
    lib.ca_copy_number_profile.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_char_p]
    lib.ca_copy_number_profile_kernel_ms.argtypes = [C.POINTER(C.c_double)]
    lib.ca_get_param.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p]
    lib.ca_set_param.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p]
    lib.ca_get_gradient.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p]
    lib.ca_reinit.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ca_get_kernel_times.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ca_reset_kernel_times.argtypes = [C.c_void_p]
    lib.ca_set_profile.argtypes = [C.c_void_p, C.c_int32]
    lib.ca_eps_draw.argtypes = [C.c_uint64, C.c_uint64, C.c_int64, C.c_void_p]
    lib.ca_preprocess.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                  C.POINTER(CaPreprocessParams), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p]
    lib.ca_allele_loglik.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                     C.c_void_p, C.c_char_p]
    lib.ca_group_create.argtypes = [C.POINTER(CaProblem), C.POINTER(CaOptions), C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    lib.ca_group_create_sparse.argtypes = [C.POINTER(CaProblem), C.POINTER(CaSparse), C.POINTER(CaOptions), C.c_void_p, C.c_int32, C.c_int32,
                                           C.POINTER(C.c_void_p)]
    lib.ca_group_destroy.argtypes = [C.c_void_p]
    lib.ca_group_get_info.argtypes = [C.c_void_p, C.POINTER(CaGroupInfo)]
    lib.ca_group_rank_handle.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    lib.ca_group_init_psi_pca.argtypes = lib.ca_init_psi_pca.argtypes
    lib.ca_group_gamma_init.argtypes = lib.ca_gamma_init.argtypes
    lib.ca_group_elbo.argtypes = lib.ca_elbo.argtypes
    lib.ca_group_step.argtypes = lib.ca_step.argtypes
    lib.ca_group_run_ex.argtypes = lib.ca_run_ex.argtypes
    lib.ca_group_iterate.argtypes = lib.ca_iterate.argtypes
    lib.ca_group_final_elbo.argtypes = lib.ca_final_elbo.argtypes
    lib.ca_group_get_param.argtypes = lib.ca_get_param.argtypes
    lib.ca_group_reinit.argtypes = lib.ca_reinit.argtypes
    lib.ca_group_clone_gene_sums.argtypes = lib.ca_clone_gene_sums.argtypes
    lib.ca_group_fit_mse.argtypes = lib.ca_fit_mse.argtypes
    lib.ca_group_logexpr_sums.argtypes = lib.ca_logexpr_sums.argtypes
    lib.ca_group_clone_loglik.argtypes = lib.ca_clone_loglik.argtypes
    lib.ca_group_project_cells.argtypes = lib.ca_project_cells.argtypes
    lib.ca_group_clone_evidence.argtypes = lib.ca_clone_evidence.argtypes
    lib.ca_group_clone_pair_loglik.argtypes = lib.ca_clone_pair_loglik.argtypes
    lib.ca_group_clone_mixture.argtypes = lib.ca_clone_mixture.argtypes
    lib.ca_group_clone_loglik_by_block.argtypes = lib.ca_clone_loglik_by_block.argtypes
    lib.ca_group_clone_loglik_dm.argtypes = lib.ca_clone_loglik_dm.argtypes
    lib.ca_clone_loglik_reweighted.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int64,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ca_group_clone_loglik_reweighted.argtypes = lib.ca_clone_loglik_reweighted.argtypes
    lib.ca_reweighted_kernel_ms.argtypes = [C.POINTER(C.c_double)]
    # initialise this library's HIP runtime NOW: torch bundles its own, and whichever runtime is loaded first must also be
    # initialised first (loaded first but initialised second it reports "no ROCm-capable device is detected")
    lib.ca_device_count(None)
    if path is None:
        _lib = lib
    return lib


def device_count():
    n = C.c_int32()
    load_library().ca_device_count(C.byref(n))
    return n.value


def _sources():
    """The library's sources in the order csrc/Makefile hashes them: every .hip / .h / .inc / .cpp of csrc/ but ca_build_id.cpp, sorted, then the C ABI."""
    import glob
    d = os.path.join(_HERE, "csrc")
    fs = sorted(f for ext in ("*.hip", "*.h", "*.inc", "*.cpp") for f in glob.glob(os.path.join(d, ext)) if os.path.basename(f) != "ca_build_id.cpp")
    return fs + [os.path.join(os.path.dirname(_HERE), "include", "clonealign_hip.h")]


def source_build_id():
    """What ca_build_id() of a library built from the sources in this tree returns (same recipe as csrc/Makefile)."""
    import hashlib
    h = hashlib.sha1()
    for f in _sources():
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def build_id():
    return load_library().ca_build_id().decode()


class EngineError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"clonealign_hip error {code}: {msg}")
        self.code = code
        self.msg = msg


_Y_DTYPES = {np.dtype(np.float64): CA_F64, np.dtype(np.float32): CA_F32, np.dtype(np.int32): CA_I32,
             np.dtype(np.uint16): CA_U16, np.dtype(np.uint8): CA_U8}


def is_sparse(a):
    """A scipy.sparse matrix / array (without importing scipy when it was never loaded: nothing else can be one)."""
    import sys
    sps = sys.modules.get("scipy.sparse")
    return sps is not None and sps.issparse(a)


def sparse_counts(Y):
    """(ca_sparse fields, arrays to keep alive) of a scipy.sparse count matrix of cells x genes: CSR and CSC go as they are (no dense
    copy); another format, or a matrix with duplicate / unsorted entries, is converted on a copy (``sum_duplicates`` also sorts).  Values
    keep their dtype when the engine takes it, else the narrowest exact one of u8 / u16 / i32, else float64."""
    if Y.format not in ("csr", "csc"):
        Y = Y.tocsr()
    if not Y.has_canonical_format:
        Y = Y.copy()
        Y.sum_duplicates()
    data = Y.data
    if data.dtype not in _Y_DTYPES:
        if data.dtype.kind in "iub" and data.size and data.min() >= 0:
            mx = int(data.max())
            dt = np.uint8 if mx <= 255 else np.uint16 if mx <= 65535 else np.int32 if mx <= np.iinfo(np.int32).max else np.float64
            data = data.astype(dt)
        else:
            data = data.astype(np.uint8 if not data.size else np.float64)
    ptr, idx = Y.indptr, Y.indices
    if ptr.dtype != idx.dtype or ptr.dtype not in (np.int32, np.int64):
        ptr, idx = ptr.astype(np.int64), idx.astype(np.int64)
    ptr, idx, data = np.ascontiguousarray(ptr), np.ascontiguousarray(idx), np.ascontiguousarray(data)
    sp = CaSparse(kind=CA_SPARSE_CSR if Y.format == "csr" else CA_SPARSE_CSC, val_dtype=_Y_DTYPES[data.dtype], index_bytes=ptr.dtype.itemsize,
                  on_device=0, nnz=int(idx.shape[0]), ptr=ptr.ctypes.data_as(C.c_void_p), idx=idx.ctypes.data_as(C.c_void_p),
                  val=data.ctypes.data_as(C.c_void_p))
    return sp, [ptr, idx, data]


def _torch_sparse_counts(Y):
    """(ca_sparse fields, tensors to keep alive) of a torch sparse CSR / CSC tensor of cells x genes on the GPU: its device arrays as
    they are (on_device = 1; index and value dtypes must be ones the engine takes)."""
    import torch
    if Y.layout == torch.sparse_csr:
        kind, ptr, idx = CA_SPARSE_CSR, Y.crow_indices(), Y.col_indices()
    elif Y.layout == torch.sparse_csc:
        kind, ptr, idx = CA_SPARSE_CSC, Y.ccol_indices(), Y.row_indices()
    else:
        raise ValueError("a torch count matrix must be dense (y_device_ptr=) or sparse CSR / CSC")
    val = Y.values()
    vdt = {torch.float64: CA_F64, torch.float32: CA_F32, torch.int32: CA_I32, torch.uint8: CA_U8}.get(val.dtype)
    if vdt is None or ptr.dtype != idx.dtype or ptr.dtype not in (torch.int32, torch.int64):
        raise ValueError("torch sparse counts: values float64 / float32 / int32 / uint8, crow / col indices both int32 or both int64")
    ptr, idx, val = ptr.contiguous(), idx.contiguous(), val.contiguous()
    torch.cuda.synchronize(Y.device)          # (the engine's runtime and stream are not torch's)
    sp = CaSparse(kind=kind, val_dtype=vdt, index_bytes=ptr.element_size(), on_device=1, nnz=int(idx.numel()),
                  ptr=C.c_void_p(ptr.data_ptr()), idx=C.c_void_p(idx.data_ptr()), val=C.c_void_p(val.data_ptr()))
    return sp, [ptr, idx, val]


def comm_unique_id():
    lib = load_library()
    buf = C.create_string_buffer(128)
    rc = lib.ca_comm_unique_id(buf)
    if rc != CA_OK:
        raise EngineError(rc, (lib.ca_last_error(None) or b"").decode())
    return bytes(buf.raw)


class HipEngine:
    """One fit on one MI355X: same constructor/method protocol as the oracle models."""

    VAR_NAMES = ("W", "v", "psi", "beta", "alpha_unconstr", "loc", "ls", "gamma_logits")
    DEVICE_MU_INIT = True   # loc0=None: mu_guess / loc0 of R/inference-tflow.R:220-235,262 from the resident matrix

    def __init__(self, Y, L, psi0, loc0, K, S=1, X=None, extra_loglik=None, learning_rate=0.1,
                 device=0, y_storage="auto", seed=0x5EED5EED, rank=0, world=1, profile=False,
                 y_device_ptr=None, y_device_dtype=None, shape=None, comm_id=None, host_allreduce=None, p2p_exchange=None,
                 layout="row", cell_index=None, gene_index=None, variant_off=(), variant_on=(), tune=None, verbose=False,
                 comm_timeout_ms=0, defer_transport=False, gate_timeout_us=0):
        """``layout``: "row" (C / numpy order) or "col" -- every matrix is then handed over column-major (Fortran order),
        which is what the R caller has (R/inference-tflow.R:190-191,355) and what r_shim/src/clonealign_hip_shim.c passes; the
        ``get``/``set`` matrices use the same layout.  ``cell_index`` / ``gene_index``: Y is the RAW matrix and the fit uses
        these rows / columns of it (ca_problem.cell_index / gene_index); L, psi0, loc0, X, extra_loglik are for the selection.
        ``p2p_exchange(handle: bytes) -> list[bytes]`` (world > 1): an all-gather of the ranks' P2P_HANDLE_BYTES-byte handles in
        rank order (torch.distributed / MPI); selects the one-shot peer-to-peer all-reduce (ca_p2p_export / ca_p2p_connect).
        ``comm_timeout_ms``: bound of the peer-to-peer all-reduce's device-side wait for its peers (0 = 10 s; ca_options).
        ``gate_timeout_us``: how long ``run``'s queued-ahead update waits on the device for the host's decision before it gives up and is
        queued again afterwards (0 = 1000 us; ca_options).
        ``Y`` may be a scipy.sparse matrix of cells x genes: CSR / CSC go to the device as their three arrays (ca_create_sparse), no dense
        copy is made, and the fit is the dense fit bit for bit.  So may a torch sparse CSR / CSC tensor on the GPU (its device arrays).
        ``variant_off``: names from VARIANTS (or a bitmask) to switch off; ``variant_on``: names from VARIANTS_ON to switch on;
        ``tune``: {name from TUNE: value}."""
        prob, opt = self._prepare(Y, L, psi0, loc0, K, S, X, extra_loglik, learning_rate, device, y_storage, seed, rank, world, profile,
                                  y_device_ptr, y_device_dtype, shape, layout, cell_index, gene_index, variant_off, variant_on, tune, verbose,
                                  comm_timeout_ms, gate_timeout_us)
        if self._sparse is not None:
            rc = self.lib.ca_create_sparse(C.byref(prob), C.byref(self._sparse), C.byref(opt), C.byref(self.h))
        else:
            rc = self.lib.ca_create(C.byref(prob), C.byref(opt), C.byref(self.h))
        if rc != CA_OK:
            msg = (self.lib.ca_last_error(None) or b"").decode()
            self.h = C.c_void_p()
            raise EngineError(rc, msg)
        if world > 1:
            if host_allreduce is not None:
                # host_allreduce(np.ndarray float64 view) must sum the array in place over all ranks
                def _cb(_user, buf, n, _f=host_allreduce):
                    try:
                        _f(np.ctypeslib.as_array(buf, shape=(n,)))
                        return 0
                    except Exception:          # never unwind through C
                        import traceback
                        traceback.print_exc()
                        return 1
                self._cb = HOST_ALLREDUCE_FN(_cb)
                self._ck(self.lib.ca_set_host_allreduce(self.h, self._cb, None))
            elif p2p_exchange is not None:
                try:
                    self._p2p_setup(p2p_exchange, world)
                except BaseException:
                    self.close()          # (frees the device resources now, not whenever the half-built object is collected)
                    raise
            elif comm_id is not None:
                self._ck(self.lib.ca_comm_init(self.h, comm_id))
            elif not defer_transport:   # (defer_transport: the caller brings the transport up itself -- _p2p_setup / comm_init)
                raise ValueError("world > 1 needs p2p_exchange, comm_id (bytes from comm_unique_id(), broadcast from rank 0) "
                                 "or host_allreduce")

    # names of the C entry points this object drives (HipGroupEngine: the ca_group_* family on a group handle)
    _PREFIX = "ca_"
    _LAST_ERROR = "ca_last_error"

    def _fn(self, name):
        return getattr(self.lib, self._PREFIX + name)

    def _prepare(self, Y, L, psi0, loc0, K, S, X, extra_loglik, learning_rate, device, y_storage, seed, rank, world, profile,
                 y_device_ptr, y_device_dtype, shape, layout, cell_index, gene_index, variant_off, variant_on, tune, verbose,
                 comm_timeout_ms, gate_timeout_us):
        """The ca_problem / ca_options of the constructor's arguments (inputs kept alive on self)."""
        self.lib = load_library()
        self.h = C.c_void_p()
        if layout not in ("row", "col"):
            raise ValueError("layout must be 'row' or 'col'")
        self.layout = CA_COL_MAJOR if layout == "col" else CA_ROW_MAJOR
        self._order = "F" if layout == "col" else "C"
        mat = lambda a, shape=None: np.require(  # noqa: E731  (a contiguous float64 matrix in the problem's layout)
            np.asarray(a, dtype=np.float64) if shape is None else np.asarray(a, dtype=np.float64).reshape(shape),
            requirements=[self._order, "A"])
        self._sparse = None
        if y_device_ptr is None and (is_sparse(Y) or "sparse_cs" in str(getattr(Y, "layout", ""))):
            # CSR / CSC arrays as they are (ca_create_sparse); Y = NULL in the problem
            Ns, Gs = (int(d) for d in Y.shape)
            self._sparse, self._keep = sparse_counts(Y) if is_sparse(Y) else _torch_sparse_counts(Y)
            y_dt, y_ptr = CA_F64, None
        elif y_device_ptr is not None:
            Ns, Gs = shape
            y_dt = _Y_DTYPES[np.dtype(y_device_dtype)]
            y_ptr = C.c_void_p(int(y_device_ptr))
            self._keep = []
        else:
            Y = np.asarray(Y)
            if Y.dtype not in _Y_DTYPES:
                Y = Y.astype(np.float64)
            Y = np.require(Y, requirements=[self._order, "A"])
            Ns, Gs = Y.shape
            y_dt = _Y_DTYPES[Y.dtype]
            y_ptr = Y.ctypes.data_as(C.c_void_p)
            self._keep = [Y]
        ci = None if cell_index is None else np.ascontiguousarray(np.asarray(cell_index, dtype=np.int64))
        gi = None if gene_index is None else np.ascontiguousarray(np.asarray(gene_index, dtype=np.int32))
        N = Ns if ci is None else ci.shape[0]
        G = Gs if gi is None else gi.shape[0]
        L = mat(L)
        self.N, self.G, self.C = int(N), int(G), int(L.shape[1])
        self.K, self.S = int(K), int(S)
        loc0 = None if loc0 is None else np.ascontiguousarray(np.asarray(loc0, dtype=np.float64))
        psi0 = mat(psi0, (self.N, self.K))
        Xc = None if X is None else mat(X, (self.N, -1))
        self.P = 0 if Xc is None else Xc.shape[1]
        ex = None if extra_loglik is None else mat(extra_loglik)
        if L.shape[0] != self.G or (loc0 is not None and loc0.shape[0] != self.G):
            raise ValueError("L / loc0 do not match the number of genes")
        self._keep += [L, loc0, psi0, Xc, ex, ci, gi]
        prob = CaProblem(N=self.N, G=self.G, C=self.C, K=self.K, P=self.P, S=self.S, layout=self.layout,
                         y_dtype=y_dt, y_on_device=int(y_device_ptr is not None), Y=y_ptr, L=_ptr(L),
                         psi0=_ptr(psi0) if self.K > 0 else None, loc0=_ptr(loc0), X=_ptr(Xc), extra_loglik=_ptr(ex),
                         N_src=int(Ns), G_src=int(Gs), cell_index=_ptr(ci), gene_index=_ptr(gi))
        opt = CaOptions()
        self.lib.ca_default_options(C.byref(opt))
        opt.learning_rate = float(learning_rate)
        opt.device = int(device)
        opt.y_storage = YSTORE[y_storage] if isinstance(y_storage, str) else int(y_storage)
        opt.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        opt.rank, opt.world = int(rank), int(world)
        opt.profile = 0x1F if profile is True else int(profile)
        opt.comm_timeout_ms = int(comm_timeout_ms)
        opt.gate_timeout_us = int(gate_timeout_us)
        voff = int(variant_off) if isinstance(variant_off, int) else sum(VARIANTS[v] for v in variant_off)
        opt.variant_off = (voff | (OPT_VERBOSE if verbose else 0)) & 0xFFFFFFFF
        opt.variant_on = int(variant_on) if isinstance(variant_on, int) else sum(VARIANTS_ON[v] for v in variant_on)
        for k, v in (tune or {}).items():
            if k in ("series_blocks", "series_side"):   # lab knobs of the series form (ca_options.reserved[0 / 1])
                opt.reserved[0 if k == "series_blocks" else 1] = int(v)
            elif k == "ride_pattern":       # (a << 8) | b, or "a:b"
                opt.ride_pattern = (lambda a, b: (int(a) << 8) | int(b))(*str(v).split(":")) if ":" in str(v) else int(v)
            else:
                opt.tune[TUNE[k]] = int(v)
        return prob, opt

    def _p2p_setup(self, p2p_exchange, world):
        """Two-phase bring-up of the one-shot peer-to-peer all-reduce (include/clonealign_hip.h): export, all-gather the handles,
        map the peers, AGREE over the control plane that every rank got that far, and only then commit -- the first call that
        waits for peers on the device.  A failure on any rank fails every rank the same way, with nobody left waiting."""
        err = None
        buf = C.create_string_buffer(P2P_HANDLE_BYTES)
        exported = self.lib.ca_p2p_export(self.h, buf) == CA_OK
        if not exported:
            err = (self.lib.ca_last_error(self.h) or b"").decode()
        allh = p2p_exchange(bytes(buf.raw) if exported else bytes(P2P_HANDLE_BYTES))
        if len(allh) != world or any(len(x) != P2P_HANDLE_BYTES for x in allh):
            raise ValueError("p2p_exchange must return one handle per rank, in rank order")
        ok = exported
        if ok and self.lib.ca_p2p_connect(self.h, b"".join(allh)) != CA_OK:
            ok, err = False, (self.lib.ca_last_error(self.h) or b"").decode()
        flags = p2p_exchange(bytes([1 if ok else 0]) + bytes(P2P_HANDLE_BYTES - 1))
        all_ok = len(flags) == world and all(len(f) > 0 and f[0] == 1 for f in flags)
        if exported:
            self._ck(self.lib.ca_p2p_commit(self.h, 1 if all_ok else 0))
        if not all_ok:
            raise EngineError(5, err or "peer-to-peer transport: another rank failed to export or map its peers")

    def comm_init(self, comm_id):
        """Join the RCCL communicator whose id rank 0 made (comm_unique_id()); collective.  Beside a committed peer-to-peer
        transport it only serves comm_benchmark("rccl"): the engine keeps reducing over peer-to-peer."""
        self._ck(self.lib.ca_comm_init(self.h, comm_id))

    def comm_benchmark(self, transport, n_calls=200, n_doubles=None):
        """us per all-reduce of ``n_doubles`` (default: the train pass's payload) on ``transport`` ("p2p" | "rccl"); collective."""
        us = C.c_double()
        n = int(self.info()["red_n"] if n_doubles is None else n_doubles)
        self._ck(self.lib.ca_comm_benchmark(self.h, {"rccl": 1, "p2p": 3}[transport], int(n_calls), n, C.byref(us)))
        return us.value

    def comm_selftest(self, n_rounds=4, n_doubles=None):
        """Known-answer test of the active all-reduce (ca_comm_selftest); returns the number of wrong sums (0 = good); collective."""
        bad = C.c_int64()
        n = int(self.info()["red_n"] if n_doubles is None else n_doubles)
        self._ck(self.lib.ca_comm_selftest(self.h, int(n_rounds), n, C.byref(bad)))
        return bad.value

    # -------------------------------------------------------------- plumbing
    def _ck(self, rc):
        if rc != CA_OK:
            raise EngineError(rc, (getattr(self.lib, self._LAST_ERROR)(self.h) or b"").decode())

    def _eps(self, eps):
        if eps is None:
            return None, None
        e = np.ascontiguousarray(np.asarray(eps, dtype=np.float32)).reshape(-1)
        if e.size != self.S * self.G:
            raise ValueError("eps must have S*G elements")
        return e, e.ctypes.data_as(C.c_void_p)

    def _stream(self, eps_stream, need):
        """eps_stream: None (built-in), ndarray [draws,S,G], or an object with .block(n)."""
        if eps_stream is None:
            return None, None, 0
        if hasattr(eps_stream, "block"):
            arr = eps_stream.block(need)
        else:
            arr = np.asarray(eps_stream, dtype=np.float32)
        arr = np.ascontiguousarray(arr, dtype=np.float32).reshape(-1, self.S * self.G)
        return arr, arr.ctypes.data_as(C.c_void_p), arr.shape[0]

    def info(self):
        i = CaInfo()
        self._ck(self.lib.ca_get_info(self.h, C.byref(i)))
        return {f[0]: getattr(i, f[0]) for f in CaInfo._fields_ if f[0] != "reserved"} | {
            "y_storage_name": YSTORE_NAME[i.y_storage], "transport_name": TRANSPORT_NAME.get(i.transport, "?")}

    # -------------------------------------------------------------- sess$run equivalents
    def gamma_init(self, eps):
        _k, p = self._eps(eps)
        self._ck(self._fn("gamma_init")(self.h, p))

    def elbo(self, eps):
        _k, p = self._eps(eps)
        out = C.c_double()
        self._ck(self._fn("elbo")(self.h, p, C.byref(out)))
        return out.value

    def elbo_terms(self, eps):
        _k, p = self._eps(eps)
        out = (C.c_double * 3)()
        self._ck(self.lib.ca_elbo_terms(self.h, p, out))
        return tuple(out)

    def step(self, eps):
        _k, p = self._eps(eps)
        self._ck(self._fn("step")(self.h, p))

    def gradients(self, eps):
        _k, p = self._eps(eps)
        out = C.c_double()
        self._ck(self.lib.ca_gradients(self.h, p, C.byref(out)))
        return {n: self._get(self.lib.ca_get_gradient, n) for n in self.VAR_NAMES}, out.value

    def last_gradients(self, names=None):
        """The gradient buffers as the last pass left them (ca_get_gradient, no ca_gradients in front): after ``iterate`` / ``run`` the gradients
        the loop's update launches applied -- include/clonealign_hip.h says which state and draw each buffer belongs to."""
        return {n: self._get(self.lib.ca_get_gradient, n) for n in (names or self.VAR_NAMES)}

    def run(self, eps_stream, max_iter, rel_tol, poll=None):
        """Whole loop of R/inference-tflow.R:368-417 in one call; returns the ELBO trace.

        ``poll(iteration, elbo)`` (optional) is called once per ELBO value as the host learns it (0 = the initial
        ELBO); a truthy return stops the loop after that iteration (ca_run_ex, CA_INTERRUPTED): the trace so far is
        returned and ``self.interrupted`` is set.  The hook may be slow and may call the read-only methods (``get``,
        ``get_params``, ``info``, ``synchronize``, ``stream_busy``): it sees the variables after that iteration, and the fit is
        the same bit for bit (include/clonealign_hip.h, ca_poll_fn); methods that change the engine's state raise from inside it."""
        need = 2 + 2 * int(max_iter)
        start = getattr(eps_stream, "draw", None)
        _k, p, n = self._stream(eps_stream, need)
        trace = np.zeros(int(max_iter) + 1, dtype=np.float64)
        cnt = C.c_int32()
        self.interrupted = False
        if poll is None:
            rc = self._fn("run_ex")(self.h, int(max_iter), float(rel_tol), p, n, trace.ctypes.data_as(C.c_void_p),
                                    C.byref(cnt), POLL_FN(0), None)
        else:
            err = []

            def _cb(_user, it, val, _f=poll):
                try:
                    return 1 if _f(int(it), float(val)) else 0
                except BaseException as e:       # never unwind through C: stop the loop, re-raise afterwards
                    err.append(e)
                    return 1
            cb = POLL_FN(_cb)
            rc = self._fn("run_ex")(self.h, int(max_iter), float(rel_tol), p, n, trace.ctypes.data_as(C.c_void_p),
                                    C.byref(cnt), cb, None)
            if err:
                raise err[0]
        if rc == CA_ERR_NAN:
            raise FloatingPointError((getattr(self.lib, self._LAST_ERROR)(self.h) or b"").decode())
        if rc == CA_INTERRUPTED:
            self.interrupted = True
        else:
            self._ck(rc)
        if start is not None:      # a stream object advances only by what the loop consumed
            eps_stream.draw = start + 2 * cnt.value
        return trace[:cnt.value].copy()

    def iterate(self, n_iter, eps_stream=None, want_elbo=True):
        _k, p, n = self._stream(eps_stream, 2 * int(n_iter))
        out = C.c_double()
        self._ck(self._fn("iterate")(self.h, int(n_iter), p, n, C.byref(out) if want_elbo else None))
        return out.value

    def final_elbo(self, eps_stream, n_rep=20):
        _k, p, n = self._stream(eps_stream, int(n_rep))
        vals = np.zeros(int(n_rep), dtype=np.float64)
        self._ck(self._fn("final_elbo")(self.h, int(n_rep), p, n, vals.ctypes.data_as(C.c_void_p), None, None))
        return vals

    def pca_init(self, noise=None, n_iter=40, seed=0):
        """psi <- scale(first K PCs of standardised log2(Y+1)) + noise, computed on the device (R/inference-tflow.R:204-208)."""
        out = np.zeros((self.N, self.K), dtype=np.float64, order=self._order)
        nz = None if noise is None else np.require(np.asarray(noise, dtype=np.float64).reshape(self.N, self.K),
                                                   requirements=[self._order, "A"])
        if self.K > 0:
            self._ck(self._fn("init_psi_pca")(self.h, _ptr(nz), int(n_iter),
                                              int(seed) & 0xFFFFFFFFFFFFFFFF, out.ctypes.data_as(C.c_void_p)))
        return out

    def clone_gene_sums(self, clone_idx):
        """(T[G,C], Syy[G]): per-gene count sums by assigned clone and sums of squares over assigned cells (-1 = unassigned)."""
        ci = np.ascontiguousarray(np.asarray(clone_idx, dtype=np.int32).reshape(self.N))
        T = np.zeros((self.G, self.C), dtype=np.float64, order=self._order)
        Syy = np.zeros(self.G, dtype=np.float64)
        self._ck(self._fn("clone_gene_sums")(self.h, ci.ctypes.data_as(C.c_void_p), T.ctypes.data_as(C.c_void_p),
                                             Syy.ctypes.data_as(C.c_void_p)))
        return T, Syy

    def fit_mse(self, clone_idx, E, per_gene=False, per_cell=False):
        """Squared error of the clones ``clone_idx`` (-1 = skip the cell) under the predicted-expression table ``E`` [G, C] (L, or mu * L), in one
        float64 sweep over the resident matrix (ca_fit_mse; R/clonealign.R:415-434).  Returns {"sse": total, "n_cells": cells used, "mse": sse /
        (n_cells * G)} plus "sse_gene" [G] / "sse_cell" [N] when asked for.  Changes nothing in the engine; two calls agree bit for bit."""
        ci = np.ascontiguousarray(np.asarray(clone_idx, dtype=np.int32).reshape(self.N))
        Em = np.require(np.asarray(E, dtype=np.float64).reshape(self.G, self.C), requirements=[self._order, "A"])
        tot, used = C.c_double(), C.c_int64()
        sg = np.zeros(self.G, dtype=np.float64) if per_gene else None
        sc = np.zeros(self.N, dtype=np.float64) if per_cell else None
        self._ck(self._fn("fit_mse")(self.h, ci.ctypes.data_as(C.c_void_p), Em.ctypes.data_as(C.c_void_p), C.byref(tot), C.byref(used), _ptr(sg), _ptr(sc)))
        out = {"sse": tot.value, "n_cells": int(used.value),
               "mse": tot.value / (used.value * self.G) if used.value > 0 and self.G > 0 else float("nan")}
        if per_gene:
            out["sse_gene"] = sg
        if per_cell:
            out["sse_cell"] = sc
        return out

    def logexpr_sums(self, group_idx, n_groups, size_factors=None):
        """Sums of the log-expression ``lc = log2(y / sf + 1)`` per gene and cell group, in one float64 sweep over the resident matrix (ca_logexpr_sums;
        the data side of plot_clonealign, R/plotting.R:177-205).  ``group_idx`` [N] in [0, n_groups), -1 = leave the cell out; ``size_factors`` [N] or
        None for library-size factors centred at 1 over the used cells.  Returns {"S1" [G, n_groups]: sums of lc per group, "S2" [G]: sums of lc^2 over
        the used cells, "n_group" [n_groups]: cells per group}.  Changes nothing in the engine; two calls agree bit for bit."""
        gi = np.ascontiguousarray(np.asarray(group_idx, dtype=np.int32).reshape(self.N))
        Q = int(n_groups)
        sf = None if size_factors is None else np.ascontiguousarray(np.asarray(size_factors, dtype=np.float64).reshape(self.N))
        S1 = np.zeros((self.G, max(Q, 0)), dtype=np.float64, order=self._order)
        S2 = np.zeros(self.G, dtype=np.float64)
        ng = np.zeros(max(Q, 0), dtype=np.int64)
        self._ck(self._fn("logexpr_sums")(self.h, gi.ctypes.data_as(C.c_void_p), Q, _ptr(sf),
                                          S1.ctypes.data_as(C.c_void_p), S2.ctypes.data_as(C.c_void_p), ng.ctypes.data_as(C.c_void_p)))
        return {"S1": S1, "S2": S2, "n_group": ng}

    def _ll_operands(self, what, E, U, V):
        """(Em, Um, Vm, D) of a log-likelihood call named ``what``: ``E`` [G, C], ``U`` [N, D] and ``V`` [G, D] in the engine's order; D = 0 passes no U, V."""
        E = np.asarray(E, dtype=np.float64)
        if E.shape != (self.G, self.C):
            raise ValueError(f"{what}: E is {E.shape} but the engine holds {self.G} genes and {self.C} clones")
        if (U is None) != (V is None):
            raise ValueError(f"{what}: U and V go together (both, or neither)")
        D = 0
        Um = Vm = None
        if U is not None:
            U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
            if U.ndim != 2 or V.ndim != 2 or U.shape[0] != self.N or V.shape[0] != self.G or U.shape[1] != V.shape[1]:
                raise ValueError(f"{what}: U is {U.shape} and V is {V.shape}; expected ({self.N}, D) and ({self.G}, D)")
            D = int(U.shape[1])
            if D > 0:
                Um, Vm = self._in_order(U), self._in_order(V)
        return self._in_order(E), Um, Vm, D

    def _latent_operands(self, what, E, V, K, X, psi_start, const, poll_every):
        """(Em, Vm, K, P, Xm, psm, flags) of a latent-factor call named ``what``: ``E`` [G, C], ``V`` [G, K + P], ``X`` [N, P] and ``psi_start`` [N, K] in
        the engine's order (None where the library takes NULL); ``flags`` = the constant's bit | ``poll_every`` << 8."""
        E = np.asarray(E, dtype=np.float64)
        if E.shape != (self.G, self.C):
            raise ValueError(f"{what}: E is {E.shape} but the engine holds {self.G} genes and {self.C} clones")
        K = int(K)
        Vm = Xm = psm = None
        D = 0
        if V is not None:
            V = np.asarray(V, dtype=np.float64)
            if V.ndim != 2 or V.shape[0] != self.G:
                raise ValueError(f"{what}: V is {V.shape}; expected ({self.G}, K + P)")
            D = int(V.shape[1])
        P = D - K
        if P < 0:
            raise ValueError(f"{what}: V has {D} columns but K = {K}")
        if D > 0:
            Vm = self._in_order(V)
        if X is not None or P > 0:
            X = np.zeros((self.N, 0)) if X is None else np.asarray(X, dtype=np.float64)
            if X.shape != (self.N, P):
                raise ValueError(f"{what}: X is {X.shape}; V has K + P = {D} columns with K = {K}, so X must be ({self.N}, {P})")
            Xm = self._in_order(X) if P > 0 else None
        if psi_start is not None and K > 0:
            psi_start = np.asarray(psi_start, dtype=np.float64)
            if psi_start.shape != (self.N, K):
                raise ValueError(f"{what}: psi_start is {psi_start.shape}; expected ({self.N}, {K})")
            psm = self._in_order(psi_start)
        if poll_every is not None and not 1 <= int(poll_every) <= 255:
            raise ValueError(f"{what}: poll_every must be in [1, 255]")
        flags = int(bool(const)) | ((int(poll_every) if poll_every is not None else 0) << 8)
        return self._in_order(E), Vm, K, P, Xm, psm, flags

    def _in_order(self, a):
        return np.require(a, requirements=[self._order, "A"])

    def _zeros(self, *shape):
        """A float64 output buffer in the engine's order."""
        return np.zeros(shape, dtype=np.float64, order=self._order)

    def _cell_range(self, cells):
        """(lo, hi, n) of ``cells`` = ``(lo, hi)`` or None for all resident cells."""
        lo, hi = (0, self.N) if cells is None else (int(cells[0]), int(cells[1]))
        return lo, hi, max(hi - lo, 0)

    def clone_loglik(self, E, U=None, V=None, const=True):
        """Log-likelihood ``ll`` [N, C] of every resident cell under every clone at point estimates, in one float64 sweep over the resident matrix
        (ca_clone_loglik; p_y_on_c of R/inference-tflow.R:288-296): ``Multinomial(total = s_n, probs ~ E[:, c] * exp(U[n] @ V.T)).log_prob(y_n)``.
        ``E`` [G, C] non-negative (a fit gives ``mu[:, None] * L``); ``U`` [N, D] and ``V`` [G, D], 0 <= D <= 8, or both None (a fit gives
        ``[psi | x]`` and ``[W | beta]``); ``const=False`` leaves out ``lgamma(s + 1) - sum(lgamma(y + 1))``.  A positive count against ``E = 0`` gives
        exactly ``-inf``, a zero count against it adds nothing; no NaN.  Changes nothing in the engine; two calls agree bit for bit."""
        Em, Um, Vm, D = self._ll_operands("clone_loglik", E, U, V)
        ll = self._zeros(self.N, self.C)
        self._ck(self._fn("clone_loglik")(self.h, _ptr(Em), _ptr(Um), _ptr(Vm), D, int(bool(const)), _ptr(ll)))
        return ll

    def clone_pair_loglik(self, E, U=None, V=None, weights=(0.5,), const=True, cells=None, want_ll=True):
        """Log-likelihood of the resident cells under every MIXTURE of two clones ``a < b`` -- a heterotypic doublet, whose counts are multinomial in
        ``w p_a + (1 - w) p_b`` -- for every weight ``w`` of ``weights`` (1 to 8 values in the open interval (0, 1); ``w`` is the share of clone ``a``), on
        the device in float64 (ca_clone_pair_loglik; include/clonealign_hip.h has the formula and the rules).  ``E``, ``U``, ``V`` and ``const`` as for
        ``clone_loglik`` (``U`` covers all resident cells); ``cells`` = ``(lo, hi)`` restricts the call to that range of cells (None: all) -- a cell's
        values do not depend on the range.  Returns ``{"ll": [n, C] (clone_loglik's rows, bit for bit; None unless want_ll), "pair_ll": [n, M, W],
        "pairs": [M, 2]}`` with the pairs in lexicographic order.  A positive count where both clones have ``E = 0`` gives exactly ``-inf``; no NaN.
        Changes nothing in the engine; two calls agree bit for bit."""
        Em, Um, Vm, D = self._ll_operands("clone_pair_loglik", E, U, V)
        lo, hi, n = self._cell_range(cells)
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1))
        Wn, Cn = int(w.shape[0]), self.C
        pairs = hostprep.pair_list(Cn)
        M = pairs.shape[0]
        ll = self._zeros(n, Cn) if want_ll else None
        pll = self._zeros(n, M * min(Wn, 8))
        self._ck(self._fn("clone_pair_loglik")(self.h, _ptr(Em), _ptr(Um), _ptr(Vm), D, int(bool(const)), _ptr(w), Wn, lo, hi - lo, _ptr(ll), _ptr(pll)))
        return {"ll": ll, "pair_ll": np.ascontiguousarray(pll).reshape(n, M, Wn), "pairs": pairs}

    def _mixture_start(self, start, lo, hi):
        """The start of a mixture call as the library takes it: the range's rows [hi - lo, C] in the engine's order."""
        return self._in_order(start)

    def clone_mixture(self, E, U=None, V=None, start=None, max_iter=50, tol=1e-3, const=True, cells=None, want_ll=True, want_grad=True):
        """The maximum-likelihood MIXTURE of all clones for each resident cell -- a spot, a bulk sample, a contaminated droplet, an off-grid doublet: counts
        multinomial in ``sum_c pi_c p_n.c`` -- on the device in float64 (ca_clone_mixture; include/clonealign_hip.h has the formulas, the round and the
        rules): simplex weights by projected Newton, stopped when the certified bound ``max_c g_c - sum_c pi_c g_c`` on what any other weights could gain
        is at most ``tol`` nats, or after ``max_iter`` rounds.  ``E``, ``U``, ``V`` and ``const`` as for ``clone_loglik`` (``U`` covers all resident
        cells; columns of ``E`` may be profiles that are no clone); ``start`` [n, C] rows on the simplex for the cells of the range, or None for uniform
        weights; ``max_iter=0`` evaluates at the start; ``cells`` = ``(lo, hi)`` restricts the call to that range (None: all) -- a cell's values do not
        depend on the range.  Returns ``{"ll": [n, C] (clone_loglik's rows, bit for bit; None unless want_ll), "weights": [n, C], "grad": [n, C]
        (``g_c / s_eff``; None unless want_grad), "mix_ll": [n], "bound": [n], "rounds": [n] int32, "converged": [n] bool (``bound <= tol``)}``.  A
        positive count that no column supports gives ``mix_ll = -inf`` exactly and is left out of the weights; no NaN.  Changes nothing in the engine;
        two calls agree bit for bit."""
        Em, Um, Vm, D = self._ll_operands("clone_mixture", E, U, V)
        lo, hi, n = self._cell_range(cells)
        Cn = self.C
        sm = None
        if start is not None:
            start = np.asarray(start, dtype=np.float64)
            if start.shape != (n, Cn):
                raise ValueError(f"clone_mixture: start is {start.shape}; expected ({n}, {Cn})")
            sm = self._mixture_start(start, lo, hi) if n > 0 else None
        ll = self._zeros(n, Cn) if want_ll else None
        w, g = self._zeros(n, Cn), (self._zeros(n, Cn) if want_grad else None)
        mll, bnd, rd = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int32)
        self._ck(self._fn("clone_mixture")(self.h, _ptr(Em), _ptr(Um), _ptr(Vm), D, int(bool(const)), _ptr(sm), int(max_iter), float(tol), lo, hi - lo, _ptr(ll),
                                           _ptr(w), _ptr(g), _ptr(mll), _ptr(bnd), _ptr(rd)))
        return {"ll": ll, "weights": np.ascontiguousarray(w), "grad": None if g is None else np.ascontiguousarray(g), "mix_ll": mll, "bound": bnd, "rounds": rd,
                "converged": bnd <= float(tol)}

    def clone_loglik_dm(self, E, U=None, V=None, concentration=(100.,), const=True, cells=None, want_ll=True):
        """DIRICHLET-MULTINOMIAL log-likelihood of the resident cells under every clone at every concentration ``phi`` of ``concentration`` (1 to 16 finite
        values > 0), on the device in float64 (ca_clone_loglik_dm; include/clonealign_hip.h has the formula and the rules):
        ``DirichletMultinomial(total = s_n, alpha = phi * p_n.c).log_prob(y_n)`` with ``p_n.c ~ E[:, c] * exp(U[n] @ V.T)`` -- ``clone_loglik``'s
        multinomial with overdispersion; ``phi -> inf`` gives it back.  ``E``, ``U``, ``V`` and ``const`` as for ``clone_loglik`` (``U`` covers all resident
        cells); ``cells`` = ``(lo, hi)`` restricts the call to that range of cells (None: all) -- a cell's values do not depend on the range.  Returns
        ``{"ll": [n, C] (clone_loglik's rows, bit for bit; None unless want_ll), "dm_ll": [n, C, n_conc]}``.  A positive count against ``E = 0`` gives
        exactly ``-inf``; no NaN.  Changes nothing in the engine; two calls agree bit for bit."""
        Em, Um, Vm, D = self._ll_operands("clone_loglik_dm", E, U, V)
        lo, hi, n = self._cell_range(cells)
        phi = np.ascontiguousarray(np.asarray(concentration, dtype=np.float64).reshape(-1))
        Kn, Cn = int(phi.shape[0]), self.C
        ll = self._zeros(n, Cn) if want_ll else None
        dm = self._zeros(n, Cn * min(Kn, 16))
        self._ck(self._fn("clone_loglik_dm")(self.h, _ptr(Em), _ptr(Um), _ptr(Vm), D, int(bool(const)), _ptr(phi), Kn, lo, hi - lo, _ptr(ll), _ptr(dm)))
        return {"ll": ll, "dm_ll": np.ascontiguousarray(dm).reshape(n, Cn, Kn)}

    def clone_loglik_by_block(self, E, U, V, block_of_gene, n_blocks, const=True, cells=None):
        """The sufficient statistics of ``clone_loglik`` BY BLOCK OF GENES (chromosomes, arms, copy-number segments), on the device in float64
        (ca_clone_loglik_by_block; include/clonealign_hip.h has the formulas and the rules).  ``E``, ``U``, ``V`` and ``const`` as for ``clone_loglik``
        (``U`` covers all resident cells; both None for D = 0); ``block_of_gene`` [G] int in ``[0, n_blocks)`` -- any labelling, interleaved labels are
        only slower; ``cells`` = ``(lo, hi)`` restricts the call to that range of cells (None: all) -- a cell's values do not depend on the range.
        Returns ``{"A": [n, B, C], "logZ": [n, B, C], "s": [n, B], "lg": [n, B] (None unless const)}``: per block ``sum xlogy(y, E) + sum y eta``,
        ``log sum E exp(eta)``, ``sum y`` and ``sum lgamma(y + 1)``.  A positive count against ``E = 0`` gives ``A = -inf`` exactly; an empty block gives
        ``A = s = lg = 0`` and ``logZ = -inf``; no NaN.  Changes nothing in the engine; two calls agree bit for bit."""
        Em, Um, Vm, D = self._ll_operands("clone_loglik_by_block", E, U, V)
        bg = np.asarray(block_of_gene)
        if bg.shape != (self.G,) or bg.dtype.kind not in "iu":
            raise ValueError(f"clone_loglik_by_block: block_of_gene must be {self.G} integers, got {bg.dtype} {bg.shape}")
        bg = np.ascontiguousarray(np.clip(bg, -1, 2 ** 31 - 1).astype(np.int32))   # (a label out of range stays out of range: the library names it)
        B = int(n_blocks)
        lo, hi, n = self._cell_range(cells)
        Bn, Cn = max(B, 0), self.C
        A, logZ, s = self._zeros(n, Bn * Cn), self._zeros(n, Bn * Cn), self._zeros(n, Bn)
        lg = self._zeros(n, Bn) if const else None
        self._ck(self._fn("clone_loglik_by_block")(self.h, _ptr(Em), _ptr(Um), _ptr(Vm), D, int(bool(const)), _ptr(bg), B, lo, hi - lo, _ptr(A), _ptr(logZ), _ptr(s), _ptr(lg)))
        return {"A": np.ascontiguousarray(A).reshape(n, Bn, Cn), "logZ": np.ascontiguousarray(logZ).reshape(n, Bn, Cn), "s": np.ascontiguousarray(s),
                "lg": None if lg is None else np.ascontiguousarray(lg)}

    def clone_loglik_reweighted(self, E, U, V, weights, log_prior=None, cells=None, want_ll=False):
        """``clone_loglik``'s score with the genes REWEIGHTED, for every row of ``weights`` [R, G] (finite, >= 0, no row all zero) at once -- the
        replicates of a bootstrap over genes -- on the device in float64 on the matrix cores (ca_clone_loglik_reweighted; include/clonealign_hip.h has the
        formulas and the rules): ``ll_r[n, c] = sum_g w_rg xlogy(y_ng, E_gc) - s_r[n] log sum_g w_rg E_gc exp(eta_ng)``, ``s_r[n] = sum_g w_rg y_ng``.  For
        integer weights that is ``clone_loglik(const=False)`` of the matrix with column g repeated ``w_rg`` times minus ``sum_g w_rg y_ng eta_ng``; that term
        and the lgamma constant are the same for every clone and are left out.  ``E``, ``U``, ``V`` as for ``clone_loglik`` (both None for D = 0; ``U``
        covers all resident cells); ``log_prior`` [N, C] over all resident cells or None (``-inf`` excludes a clone); ``cells`` = ``(lo, hi)`` restricts
        the call to that range (None: all).  Returns ``{"votes": [n, C] int32 (replicates whose argmax of ll_r + log_prior is c, ties to the lowest),
        "prob_sum", "prob_sq": [n, C] (sums over r of the softmax and of its square), "reads": [n, R] (s_r), "ll": [n, R, C] (None unless want_ll)}``.
        ``ll_r = -inf`` exactly where a positive count with a positive weight meets ``E = 0``; ``s_r = 0`` gives ``ll_r = 0``; no NaN.  No value depends
        on the cell range, the batching or on which other replicates share the call.  Changes nothing in the engine; two calls agree bit for bit."""
        Em, Um, Vm, D = self._ll_operands("clone_loglik_reweighted", E, U, V)
        lo, hi, n = self._cell_range(cells)
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64))
        if w.ndim != 2 or w.shape[1] != self.G:
            raise ValueError(f"clone_loglik_reweighted: weights is {w.shape}; expected (R, {self.G})")
        R, Cn = int(w.shape[0]), self.C
        lpm = None
        if log_prior is not None:
            log_prior = np.asarray(log_prior, dtype=np.float64)
            if log_prior.shape != (self.N, Cn):
                raise ValueError(f"clone_loglik_reweighted: log_prior is {log_prior.shape}; expected ({self.N}, {Cn})")
            lpm = self._in_order(log_prior)
        ll = self._zeros(n, R * Cn) if want_ll else None
        ps, pq, rd = self._zeros(n, Cn), self._zeros(n, Cn), self._zeros(n, R)
        votes = np.zeros((n, Cn), dtype=np.int32, order=self._order)
        self._ck(self._fn("clone_loglik_reweighted")(self.h, _ptr(Em), _ptr(Um), _ptr(Vm), D, _ptr(w), R, _ptr(lpm), lo, hi - lo, _ptr(ll), _ptr(votes), _ptr(ps),
                                                     _ptr(pq), _ptr(rd)))
        return {"votes": np.ascontiguousarray(votes), "prob_sum": np.ascontiguousarray(ps), "prob_sq": np.ascontiguousarray(pq), "reads": np.ascontiguousarray(rd),
                "ll": None if ll is None else np.ascontiguousarray(ll).reshape(n, R, Cn)}

    def project_cells(self, E, V=None, K=0, X=None, log_prior=None, psi_start=None, const=True, max_iter=25, tol=1e-9, max_step=1.0, poll_every=None):
        """Per-cell MAP ``psi`` of the resident cells under a fit's gene-level parameters and the exact clone posterior at it (ca_project_cells;
        include/clonealign_hip.h has the algorithm): maximises ``logsumexp_c(ll_nc(psi) + log_prior_nc) - |psi|^2 / 2`` per cell by generalised EM with one
        safeguarded Newton step per round.  ``E`` [G, C]; ``V`` = ``[W | beta]`` [G, K + P] with ``K`` <= 2 free factors (the device limit); ``X`` [N, P];
        ``log_prior`` [N, C] (``log alpha + extra``; ``-inf`` excludes a clone) or None; ``psi_start`` [N, K] or None = 0.  One sweep over the resident
        matrix, then two launches per round that do not read it.  Returns a dict: ``psi`` [N, K], ``ll`` and ``clone_probs`` [N, C], ``objective`` [N],
        ``rounds`` [N] int32, ``converged`` [N] bool.  ``poll_every``: rounds between two host reads of the frozen flags (None = 4); no result depends
        on it.  Changes nothing in the engine; two calls agree bit for bit."""
        Em, Vm, K, P, Xm, psm, flags = self._latent_operands("project_cells", E, V, K, X, psi_start, const, poll_every)
        lpm = None
        if log_prior is not None:
            log_prior = np.asarray(log_prior, dtype=np.float64)
            if log_prior.shape != (self.N, self.C):
                raise ValueError(f"project_cells: log_prior is {log_prior.shape}; expected ({self.N}, {self.C})")
            lpm = self._in_order(log_prior)
        psi, ll, pr, obj = self._zeros(self.N, max(K, 0)), self._zeros(self.N, self.C), self._zeros(self.N, self.C), self._zeros(self.N)
        rounds = np.zeros(self.N, dtype=np.int32)
        conv = np.zeros(self.N, dtype=np.uint8)
        self._ck(self._fn("project_cells")(self.h, _ptr(Em), _ptr(Vm), K, P, _ptr(Xm), _ptr(lpm), _ptr(psm), flags, int(max_iter), float(tol), float(max_step),
                                           _ptr(psi) if K > 0 else None, _ptr(ll), _ptr(pr), _ptr(obj), _ptr(rounds), _ptr(conv)))
        return {"psi": psi, "ll": ll, "clone_probs": pr, "objective": obj, "rounds": rounds, "converged": conv.astype(bool)}

    def clone_evidence(self, E, V=None, K=0, X=None, psi_start=None, nodes=None, weights=None, const=True, max_iter=50, tol=1e-9, max_step=1.0,
                       poll_every=None):
        """Clone evidence of the resident cells with ``psi`` integrated out (ca_clone_evidence; include/clonealign_hip.h has the algorithm): per (cell,
        clone) the mode of ``f(psi) = log Multinomial(y | c, psi) - |psi|^2 / 2`` by safeguarded Newton, the Laplace value and a quadrature at the caller's
        rule for the standard normal measure, centred at the mode and scaled by the Cholesky factor of the precision.  ``E`` [G, C]; ``V`` = ``[W | beta]``
        [G, K + P] with ``K`` <= 2 free factors (the device limit); ``X`` [N, P]; ``psi_start`` [N, K] or None = 0 (one start for every clone); ``nodes``
        [Q, K] and ``weights`` [Q] (``api.gauss_hermite_rule``; None: the single node 0, the Laplace value), Q <= 64.  One sweep over the resident matrix,
        then launches that do not read it.  Returns a dict: ``evidence`` and ``laplace`` [N, C], ``psi_mode`` [N, C, K], ``psi_prec`` [N, C, K (K + 1) / 2]
        (the precision's entries k <= l), ``rounds`` [N, C] int32, ``converged`` [N, C] bool -- a pair with ``converged`` False holds a value that is
        deterministic but not to be trusted.  ``poll_every``: rounds between two host reads of the pairs' states (None = 4); no result depends on it.
        Changes nothing in the engine; two calls agree bit for bit."""
        Em, Vm, K, P, Xm, psm, flags = self._latent_operands("clone_evidence", E, V, K, X, psi_start, const, poll_every)
        if (nodes is None) != (weights is None):
            raise ValueError("clone_evidence: nodes and weights go together (both, or neither)")
        if nodes is None:
            nodes, weights = np.zeros((1, max(K, 0))), np.ones(1)
        wts = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        nd = np.ascontiguousarray(nodes, dtype=np.float64)             # (row-major always: node by node)
        Q = int(wts.shape[0])
        if nd.size != Q * max(K, 0):
            raise ValueError(f"clone_evidence: nodes is {nd.shape}; {Q} weights and K = {K} need ({Q}, {K})")
        Kp = max(K, 0)
        NH = Kp * (Kp + 1) // 2
        ev, lap, mode, prec = self._zeros(self.N, self.C), self._zeros(self.N, self.C), self._zeros(self.N, self.C * Kp), self._zeros(self.N, self.C * NH)
        rounds = np.zeros((self.N, self.C), dtype=np.int32, order=self._order)
        conv = np.zeros((self.N, self.C), dtype=np.uint8, order=self._order)
        Em, Vm, Xm, psm, nd_p, wts_p, *outs = (_ptr(a, empty_null=True) for a in (Em, Vm, Xm, psm, nd, wts, ev, lap, mode, prec, rounds, conv))   # (K = 0: no nodes, modes)
        self._ck(self._fn("clone_evidence")(self.h, Em, Vm, K, P, Xm, psm, flags, Q, nd_p, wts_p, int(max_iter), float(tol), float(max_step), *outs))
        return {"evidence": np.ascontiguousarray(ev), "laplace": np.ascontiguousarray(lap), "psi_mode": np.ascontiguousarray(mode).reshape(self.N, self.C, Kp),
                "psi_prec": np.ascontiguousarray(prec).reshape(self.N, self.C, NH), "rounds": np.ascontiguousarray(rounds),
                "converged": np.ascontiguousarray(conv).astype(bool)}

    def synchronize(self):
        self._ck(self.lib.ca_synchronize(self.h))

    def stream_busy(self):
        """True while work queued on the engine's stream has not completed (ca_stream_busy; never blocks)."""
        b = C.c_int32()
        self._ck(self.lib.ca_stream_busy(self.h, C.byref(b)))
        return bool(b.value)

    def ystream_parts(self):
        """What the count-matrix stream's last launch left, before its finisher (ca_ystream_parts; read-only): ``yw_part`` [nseg, N] and ``yt_part`` [nrg, Gp]
        float32, ``exps`` (W, psi), ``strip_cells`` (a row group of yt_part is four strips), the fixed-point values in the parameter images now (``w_fix`` [Gp], ``p_fix`` [N64], int32) and ``images_current`` -- whether
        those are the images that launch read.  include/clonealign_hip.h states each."""
        dims = (C.c_int64 * 6)()
        self._ck(self.lib.ca_ystream_parts(self.h, dims, None, None, None, None, None))
        nseg, N, nrg, Gp, RS, _cur = (int(d) for d in dims)
        N64 = -(-N // 64) * 64
        yw, yt = np.empty((nseg, N), np.float32), np.empty((nrg, Gp), np.float32)
        exps, wf, pf = np.empty(2, np.int32), np.empty(Gp, np.int32), np.empty(N64, np.int32)
        self._ck(self.lib.ca_ystream_parts(self.h, dims, *(a.ctypes.data_as(C.c_void_p) for a in (yw, yt, exps, wf, pf))))
        return {"yw_part": yw, "yt_part": yt, "exps": exps, "w_fix": wf, "p_fix": pf, "strip_cells": RS, "images_current": bool(dims[5])}

    # -------------------------------------------------------------- fetch / poke
    def _shape(self, name):
        N, G, Cn, K, P = self.N, self.G, self.C, self.K, self.P
        return {"mu": (G,), "loc": (G,), "ls": (G,), "clone_probs": (N, Cn), "gamma_logits": (N, Cn), "s": (N,),
                "alpha": (Cn,), "alpha_unconstr": (Cn,), "beta": (G, P), "psi": (N, K), "W": (G, K),
                "chi": (K,), "v": (K,)}[name]

    def _get(self, fn, name):
        out = np.zeros(self._shape(name), dtype=np.float64, order=self._order)   # the library writes the problem's layout
        if out.size:
            self._ck(fn(self.h, name.encode(), out.ctypes.data_as(C.c_void_p)))
        return out

    def get(self, name):
        return self._get(self._fn("get_param"), name)

    def set(self, name, value):
        v = np.require(np.asarray(value, dtype=np.float64).reshape(self._shape(name)), requirements=[self._order, "A"])
        if v.size:
            self._ck(self.lib.ca_set_param(self.h, name.encode(), v.ctypes.data_as(C.c_void_p)))

    def reinit(self, psi0, loc0=None):
        """A new restart on the resident data: variables back to their initial values (psi = psi0, loc = loc0 or what the
        constructor started from), fresh Adam state (ca_reinit)."""
        p0 = None
        if self.K > 0:
            p0 = np.require(np.asarray(psi0, dtype=np.float64).reshape(self.N, self.K), requirements=[self._order, "A"])
        l0 = None if loc0 is None else np.ascontiguousarray(np.asarray(loc0, dtype=np.float64).reshape(self.G))
        self._ck(self._fn("reinit")(self.h, _ptr(p0), _ptr(l0)))

    def get_params(self):
        """R/inference-tflow.R:424-434."""
        out = {n: self.get(n) for n in ("mu", "clone_probs", "s", "alpha")}
        if self.P > 0:
            out["beta"] = self.get("beta")
        if self.K > 0:
            for n in ("psi", "W", "chi"):
                out[n] = self.get(n)
        return out

    def get_state(self):
        return {n: self.get(n) for n in self.VAR_NAMES}

    def kernel_times(self, reset=False):
        ms = (C.c_double * 5)()
        cnt = (C.c_int64 * 5)()
        self._ck(self.lib.ca_get_kernel_times(self.h, ms, cnt))
        if reset:
            self._ck(self.lib.ca_reset_kernel_times(self.h))
        return {k: (ms[i], cnt[i]) for i, k in enumerate(KERNEL_NAMES)}

    def set_profile(self, mask):
        self._ck(self.lib.ca_set_profile(self.h, int(mask)))

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self._fn("destroy")(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HipGroupEngine(HipEngine):
    """ONE fit cell-sharded over several devices of this process (ca_group_*, include/clonealign_hip.h ABI 6): the engine behind
    ``inference_tflow(..., devices=[...])``.  Same constructor arguments as :class:`HipEngine` for ALL cells, plus ``devices`` (HIP
    ordinals in rank order; an ordinal may repeat on a one-GPU rig) and ``transport`` ("auto": peer-to-peer by address -> RCCL -> host
    reduction between the rank threads, each after a known-answer test; or one of "p2p" / "rccl" / "host" to insist on it).  Every method returns
    what the one-handle method returns for all cells.  Calls that have no group form (gradients, set, kernel_times ...) raise."""

    _PREFIX = "ca_group_"
    _LAST_ERROR = "ca_group_last_error"
    _TRANSPORT = {"auto": 0, "rccl": 1, "host": 2, "p2p": 3}

    def __init__(self, Y, L, psi0, loc0, K, S=1, X=None, extra_loglik=None, learning_rate=0.1, devices=(0,), transport="auto",
                 y_storage="auto", seed=0x5EED5EED, profile=False, y_device_ptr=None, y_device_dtype=None, shape=None, layout="row",
                 cell_index=None, gene_index=None, variant_off=(), variant_on=(), tune=None, verbose=False, comm_timeout_ms=0, gate_timeout_us=0):
        prob, opt = self._prepare(Y, L, psi0, loc0, K, S, X, extra_loglik, learning_rate, 0, y_storage, seed, 0, 1, profile,
                                  y_device_ptr, y_device_dtype, shape, layout, cell_index, gene_index, variant_off, variant_on, tune, verbose,
                                  comm_timeout_ms, gate_timeout_us)
        self.devices = [int(d) for d in devices]
        dev = (C.c_int32 * len(self.devices))(*self.devices)
        if self._sparse is not None:
            rc = self.lib.ca_group_create_sparse(C.byref(prob), C.byref(self._sparse), C.byref(opt), dev, len(self.devices),
                                                 self._TRANSPORT[transport], C.byref(self.h))
        else:
            rc = self.lib.ca_group_create(C.byref(prob), C.byref(opt), dev, len(self.devices), self._TRANSPORT[transport], C.byref(self.h))
        if rc != CA_OK:
            msg = (self.lib.ca_group_last_error(None) or b"").decode()
            self.h = C.c_void_p()
            raise EngineError(rc, msg)

    def group_info(self):
        i = CaGroupInfo()
        self._ck(self.lib.ca_group_get_info(self.h, C.byref(i)))
        return {"world": i.world, "transport": i.transport, "transport_name": TRANSPORT_NAME.get(i.transport, "?"), "p2p_status": i.p2p_status,
                "rccl_status": i.rccl_status, "rebuilds": i.rebuilds, "selftest_rounds": i.selftest_rounds, "N": i.N, "note": i.note.decode()}

    def rank_info(self, rank):
        """ca_get_info of one rank's engine (its shard's cells, its kernel picks)."""
        h = C.c_void_p()
        self._ck(self.lib.ca_group_rank_handle(self.h, int(rank), C.byref(h)))
        i = CaInfo()
        rc = self.lib.ca_get_info(h, C.byref(i))
        if rc != CA_OK:
            raise EngineError(rc, "ca_get_info")
        return {f[0]: getattr(i, f[0]) for f in CaInfo._fields_} | {"y_storage_name": YSTORE_NAME[i.y_storage],
                                                                    "transport_name": TRANSPORT_NAME.get(i.transport, "?")}

    def rank_last_gradients(self, rank, names=None):
        """``HipEngine.last_gradients`` of one rank's engine (ca_get_gradient on the rank handle; read-only, runs nothing): psi and gamma_logits for the rank's
        own cells, every other variable whole.  Between two group calls no rank thread touches its engine, so the read from the calling thread is safe."""
        h = C.c_void_p()
        self._ck(self.lib.ca_group_rank_handle(self.h, int(rank), C.byref(h)))
        i = CaInfo()
        rc = self.lib.ca_get_info(h, C.byref(i))
        if rc != CA_OK:
            raise EngineError(rc, "ca_get_info")
        out = {}
        for name in (names or self.VAR_NAMES):
            shape = tuple(int(i.N) if (d == 0 and name in ("psi", "gamma_logits")) else s for d, s in enumerate(self._shape(name)))
            a = np.zeros(shape, dtype=np.float64, order=self._order)
            if a.size:
                rc = self.lib.ca_get_gradient(h, name.encode(), a.ctypes.data_as(C.c_void_p))
                if rc != CA_OK:
                    raise EngineError(rc, (self.lib.ca_last_error(h) or b"").decode())
            out[name] = a
        return out

    def info(self):
        return self.rank_info(0) | {"N": self.N, "group": self.group_info()}

    def _mixture_start(self, start, lo, hi):
        """ca_group_clone_mixture takes the start over ALL cells, as it takes U: the range's rows in place, the others unread."""
        full = self._zeros(self.N, self.C)
        if 0 <= lo <= hi <= self.N:                                  # (any other range is the library's to refuse)
            full[lo:hi] = start
        return full

    def clone_mixture(self, E, U=None, V=None, start=None, max_iter=50, tol=1e-3, const=True, cells=None, want_ll=True, want_grad=True):
        """``HipEngine.clone_mixture`` over the group (ca_group_clone_mixture): every rank solves the cells of the range that lie in its shard; each cell's
        values are the single handle's, bit for bit."""
        return super().clone_mixture(E, U, V, start=start, max_iter=max_iter, tol=tol, const=const, cells=cells, want_ll=want_ll, want_grad=want_grad)

    def _no(self, *a, **k):
        raise NotImplementedError("not available on a device group (use the rank engines through rank_info / a single HipEngine)")

    elbo_terms = gradients = last_gradients = set = kernel_times = set_profile = synchronize = stream_busy = _no
    comm_init = comm_benchmark = comm_selftest = _no


def eps_draw(seed, draw, n):
    """The library's built-in eps stream (host side), for checking against rng.normal_draw."""
    lib = load_library()
    out = np.zeros(int(n), dtype=np.float32)
    rc = lib.ca_eps_draw(int(seed), int(draw), int(n), out.ctypes.data_as(C.c_void_p))
    if rc != CA_OK:
        raise EngineError(rc, "ca_eps_draw")
    return out


def _lay(layout):
    if layout not in ("row", "col"):
        raise ValueError("layout must be 'row' or 'col'")
    return (CA_COL_MAJOR, "F") if layout == "col" else (CA_ROW_MAJOR, "C")


def allele_loglik(clone_allele, cov, ref, device=0, layout="row"):
    """The allele-specific [N, C] addend of the log-likelihood on the device (ca_allele_loglik; R/allele-specific.R:17-58
    with alt = cov - ref as at R/inference-tflow.R:173).  clone_allele [V, C]; cov, ref [N, V].  ``layout="col"`` hands the
    matrices over column-major, as the R caller would."""
    lib = load_library()
    lay, order = _lay(layout)
    req = [order, "A"]
    ca = np.require(np.asarray(clone_allele, dtype=np.float64), requirements=req)
    cv = np.require(np.asarray(cov, dtype=np.float64), requirements=req)
    rf = np.require(np.asarray(ref, dtype=np.float64), requirements=req)
    V, Cn = ca.shape
    N = cv.shape[0]
    if cv.shape != (N, V) or rf.shape != (N, V):
        raise ValueError("cov and ref must be cells x variants, clone_allele variants x clones")
    out = np.zeros((N, Cn), dtype=np.float64, order=order)
    err = C.create_string_buffer(256)
    rc = lib.ca_allele_loglik(N, V, Cn, lay, ca.ctypes.data_as(C.c_void_p), cv.ctypes.data_as(C.c_void_p),
                              rf.ctypes.data_as(C.c_void_p), int(device), out.ctypes.data_as(C.c_void_p), err)
    if rc != CA_OK:
        raise EngineError(rc, err.value.decode() or "ca_allele_loglik")
    return out


def _model_operands(what, E, V, U, clone, total):
    """The model arguments the handle-free generative calls share, as the library reads them: ``(E, V, U, clone, total, N, G, Cn, D)`` with C-contiguous float64
    ``E`` [G, Cn], int32 ``clone`` [N] and int64 ``total`` [N] (a scalar is every cell's); ``V`` [G, D] and ``U`` [N, D] float64, or both None where D = 0."""
    E = np.ascontiguousarray(E, dtype=np.float64)
    if E.ndim != 2:
        raise ValueError(f"{what}: E is {E.shape}; expected (genes, clones)")
    G, Cn = E.shape
    clone = np.ascontiguousarray(clone, dtype=np.int32).reshape(-1)
    N = clone.shape[0]
    total = np.ascontiguousarray(np.broadcast_to(np.asarray(total, dtype=np.int64), (N,)))
    if (U is None) != (V is None):
        raise ValueError(f"{what}: U and V go together (both, or neither)")
    D = 0
    if U is not None:
        U, V = np.ascontiguousarray(U, dtype=np.float64), np.ascontiguousarray(V, dtype=np.float64)
        if U.ndim != 2 or V.ndim != 2 or U.shape[0] != N or V.shape[0] != G or U.shape[1] != V.shape[1]:
            raise ValueError(f"{what}: U is {U.shape} and V is {V.shape}; expected ({N}, D) and ({G}, D)")
        D = int(U.shape[1])
    if D == 0:
        U = V = None
    return E, V, U, clone, total, N, G, Cn, D


def _last_kernel_ms(symbol):
    ms = C.c_double(0.0)
    getattr(load_library(), symbol)(C.byref(ms))
    return ms.value


def simulate_counts(E, V, U, clone, total, seed, draw=0, cell_offset=0, device=0, out=None):
    """Count rows drawn from a fitted model on the device (ca_simulate_counts; include/clonealign_hip.h has the sampler): ``y_n ~ Multinomial(total[n],
    p_n)``, ``p_ng ~ E[g, clone[n]] exp(U[n] . V[g])``.  ``E`` [G, C]; ``V`` [G, D] and ``U`` [N, D], or both None; ``clone`` [N] in [0, C); ``total`` [N].
    Returns int32 [N, G] (``out``: a C-contiguous int32 [N, G] array to fill instead).  Row n depends on (seed, draw, cell_offset + n) and its own
    arguments alone, so splitting the cells over calls (or devices) with ``cell_offset`` gives the same bits.  Refusals raise EngineError."""
    lib = load_library()
    E, V, U, clone, total, N, G, Cn, D = _model_operands("simulate_counts", E, V, U, clone, total)
    if out is None:
        out = np.zeros((N, G), dtype=np.int32)
    elif out.dtype != np.int32 or out.shape != (N, G) or not out.flags.c_contiguous:
        raise ValueError(f"simulate_counts: out must be a C-contiguous int32 array of shape ({N}, {G})")
    err = C.create_string_buffer(256)
    rc = lib.ca_simulate_counts(N, G, Cn, D, _ptr(E), _ptr(V), _ptr(U), _ptr(clone), _ptr(total),
                                int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw) & 0xFFFFFFFFFFFFFFFF, int(cell_offset), int(device), _ptr(out), err)
    if rc != CA_OK:
        raise EngineError(rc, err.value.decode() or "ca_simulate_counts")
    return out


def simulate_kernel_ms():
    """Milliseconds the kernel launches of this thread's last ``simulate_counts`` call took (HIP events around each launch)."""
    return _last_kernel_ms("ca_simulate_kernel_ms")


def reweighted_kernel_ms():
    """Milliseconds the kernel launches of this thread's last ``HipEngine.clone_loglik_reweighted`` call took (HIP events around the launches, no copy)."""
    return _last_kernel_ms("ca_reweighted_kernel_ms")


def predictive_stats(E, V, U, clone, total, seed, draw0=0, n_rep=1, cell_offset=0, device=0, gene_totals=True, out=None):
    """Statistics of ``n_rep`` replicate rows of ``simulate_counts`` without the rows (ca_predictive_stats; include/clonealign_hip.h states them): replicate
    ``r`` is the matrix ``simulate_counts(..., seed, draw=draw0 + r, cell_offset)`` returns, drawn and reduced on the device.  Arguments as for
    ``simulate_counts``.  Returns ``(ll_rep, T_rep)``: ``ll_rep`` float64 [N, n_rep], the multinomial log-probability of each replicate row under the
    cell's own ``p``; ``T_rep`` int64 [n_rep, G, C], the rows summed per clone (None with ``gene_totals=False``).  ``out``: a pair of C-contiguous arrays
    of these shapes and dtypes to fill instead (the second None without totals).  ``ll_rep[n, r]`` depends on (seed, draw0 + r, cell_offset + n) and the
    cell's own arguments alone; ``T_rep`` of cells split over calls adds up.  Refusals raise EngineError."""
    lib = load_library()
    E, V, U, clone, total, N, G, Cn, D = _model_operands("predictive_stats", E, V, U, clone, total)
    n_rep = int(n_rep)
    if not -2 ** 31 <= n_rep < 2 ** 31:
        raise ValueError(f"predictive_stats: n_rep = {n_rep} does not fit 32 bits")
    R = max(n_rep, 0)
    if out is None:
        ll, T = np.zeros((N, R), dtype=np.float64), (np.zeros((R, G, Cn), dtype=np.int64) if gene_totals else None)
    else:
        ll, T = out
        if ll.dtype != np.float64 or ll.shape != (N, R) or not ll.flags.c_contiguous:
            raise ValueError(f"predictive_stats: out[0] must be a C-contiguous float64 array of shape ({N}, {R})")
        if T is not None and (T.dtype != np.int64 or T.shape != (R, G, Cn) or not T.flags.c_contiguous):
            raise ValueError(f"predictive_stats: out[1] must be None or a C-contiguous int64 array of shape ({R}, {G}, {Cn})")
    err = C.create_string_buffer(256)
    rc = lib.ca_predictive_stats(N, G, Cn, D, _ptr(E), _ptr(V), _ptr(U), _ptr(clone), _ptr(total),
                                 int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw0) & 0xFFFFFFFFFFFFFFFF, n_rep, int(cell_offset), int(device), _ptr(ll), _ptr(T), err)
    if rc != CA_OK:
        raise EngineError(rc, err.value.decode() or "ca_predictive_stats")
    return ll, T


def predictive_kernel_ms():
    """Milliseconds the kernel launches of this thread's last ``predictive_stats`` call took (HIP events around each launch)."""
    return _last_kernel_ms("ca_predictive_kernel_ms")


def predictive_moments(E, V, U, clone, total, device=0):
    """The moments of ``predictive_stats``'s replicates in closed form, nothing drawn (ca_predictive_moments; include/clonealign_hip.h states them).  Arguments
    as for ``simulate_counts``.  Returns ``(cell_mean, cell_var, T_mean, T_var, T_cum3)``: per cell the mean and variance over the replicates of the linear
    part of the row's log-likelihood, ``sum_g y_g log p_g`` (float64 [N]); per (gene, clone) the mean, variance and third cumulant of the rows summed per
    clone (float64 [G, C]).  The cell values depend on the cell's own arguments alone; the tables of cells split over calls add up to within rounding.
    Refusals raise EngineError."""
    lib = load_library()
    E, V, U, clone, total, N, G, Cn, D = _model_operands("predictive_moments", E, V, U, clone, total)
    cell = np.zeros((2, max(N, 1)), dtype=np.float64)                # (never an empty buffer: the call wants five pointers also without cells)
    T = np.zeros((3, G, Cn), dtype=np.float64)
    err = C.create_string_buffer(256)
    rc = lib.ca_predictive_moments(N, G, Cn, D, _ptr(E), _ptr(V), _ptr(U), _ptr(clone), _ptr(total), int(device),
                                   _ptr(cell[0]), _ptr(cell[1]), _ptr(T[0]), _ptr(T[1]), _ptr(T[2]), err)
    if rc != CA_OK:
        raise EngineError(rc, err.value.decode() or "ca_predictive_moments")
    return cell[0, :N], cell[1, :N], T[0], T[1], T[2]


def predictive_moments_kernel_ms():
    """Milliseconds the kernel launches of this thread's last ``predictive_moments`` call took (HIP events around each launch; 0 without factors)."""
    return _last_kernel_ms("ca_predictive_moments_kernel_ms")


def clone_separability(E, V, U, device=0):
    """How well expression separates every ordered pair of clones, per cell, in closed form; no counts are read (ca_clone_separability;
    include/clonealign_hip.h states the outputs).  ``E`` [G, C]; ``V`` [G, D] and ``U`` [N, D]: one row per cell.  Without factors (both None) the values do not
    depend on the cell and one row is returned.  Returns ``(logZ [N, C], excl, m1, m2, m3 [N, C, C])``, float64: for a row of clone ``a`` against clone ``b``
    the per-read probability of a read that excludes ``b`` and the first three per-read moments of the log-likelihood ratio over the genes both clones
    express.  A cell's values depend on its own row of ``U`` alone, so cells may be split over calls or devices.  Refusals raise EngineError."""
    lib = load_library()
    E = np.ascontiguousarray(E, dtype=np.float64)
    if E.ndim != 2:
        raise ValueError(f"clone_separability: E is {E.shape}; expected (genes, clones)")
    G, Cn = E.shape
    if (U is None) != (V is None):
        raise ValueError("clone_separability: U and V go together (both, or neither)")
    N, D = 1, 0
    if U is not None:
        U, V = np.ascontiguousarray(U, dtype=np.float64), np.ascontiguousarray(V, dtype=np.float64)
        if U.ndim != 2 or V.ndim != 2 or V.shape[0] != G or U.shape[1] != V.shape[1]:
            raise ValueError(f"clone_separability: U is {U.shape} and V is {V.shape}; expected (cells, D) and ({G}, D)")
        N, D = int(U.shape[0]), int(U.shape[1])
        if D == 0:
            U = V = None
    logZ = np.zeros((max(N, 1), Cn), dtype=np.float64)               # (never an empty buffer: the call wants five pointers also without cells)
    pair = np.zeros((4, max(N, 1), Cn, Cn), dtype=np.float64)
    err = C.create_string_buffer(256)
    rc = lib.ca_clone_separability(N, G, Cn, D, _ptr(E), _ptr(V), _ptr(U), int(device), _ptr(logZ), _ptr(pair[0]), _ptr(pair[1]), _ptr(pair[2]), _ptr(pair[3]), err)
    if rc != CA_OK:
        raise EngineError(rc, err.value.decode() or "ca_clone_separability")
    return logZ[:N], pair[0, :N], pair[1, :N], pair[2, :N], pair[3, :N]


def clone_separability_kernel_ms():
    """Milliseconds the kernel launches of this thread's last ``clone_separability`` call took (HIP events around each launch; 0 without factors)."""
    return _last_kernel_ms("ca_clone_separability_kernel_ms")


def copy_number_profile(E, V, U, clone, total, mu, kappa, blocks=None, device=0):
    """The expression side of the likelihood profile over the copy-number matrix (ca_copy_number_profile; include/clonealign_hip.h states it): ``cost[b, c, j]``
    = the sum over the cells of clone ``c`` of ``total log1p(sum_{g in b} (mu_g kappa_j - E[g, c]) x_ng)``, what replacing ``E[g, c]`` by ``mu_g kappa_j`` for the
    genes of block ``b`` adds to the cells' ``total log Z``.  Arguments as for ``predictive_moments``; ``mu`` [G] and ``kappa`` [J], 1 <= J <= 16, finite and
    >= 0; ``blocks``: None (per-gene mode, every gene its own block) or int labels [G] in [0, B) with B = the largest label + 1, at most 2048.  Returns float64
    [G or B, C, J].  No counts are read; the tables of cells split over calls add up to within rounding.  Refusals raise EngineError."""
    lib = load_library()
    E, V, U, clone, total, N, G, Cn, D = _model_operands("copy_number_profile", E, V, U, clone, total)
    mu = np.ascontiguousarray(mu, dtype=np.float64).reshape(-1)
    kappa = np.ascontiguousarray(kappa, dtype=np.float64).reshape(-1)
    if mu.shape[0] != G:
        raise ValueError(f"copy_number_profile: mu has {mu.shape[0]} entries but E has {G} rows (genes)")
    B = G
    if blocks is not None:
        blocks = np.ascontiguousarray(blocks, dtype=np.int32).reshape(-1)
        if blocks.shape[0] != G:
            raise ValueError(f"copy_number_profile: blocks has {blocks.shape[0]} labels but E has {G} rows (genes)")
        B = int(blocks.max()) + 1 if G else 0
    cost = np.zeros((max(B, 1), Cn, max(kappa.shape[0], 1)), dtype=np.float64)      # (never an empty buffer; a refused B or J leaves it unread)
    err = C.create_string_buffer(256)
    rc = lib.ca_copy_number_profile(N, G, Cn, D, _ptr(E), _ptr(V), _ptr(U), _ptr(clone), _ptr(total), _ptr(mu), int(kappa.shape[0]), _ptr(kappa),
                                    B, _ptr(blocks), int(device), _ptr(cost), err)
    if rc != CA_OK:
        raise EngineError(rc, err.value.decode() or "ca_copy_number_profile")
    return cost


def copy_number_profile_kernel_ms():
    """Milliseconds the kernel launches of this thread's last ``copy_number_profile`` call took (HIP events around each launch; 0 without factors)."""
    return _last_kernel_ms("ca_copy_number_profile_kernel_ms")


_NP_DTYPE = {np.dtype(np.float64): 0, np.dtype(np.float32): 1, np.dtype(np.int32): 2, np.dtype(np.uint16): 3, np.dtype(np.uint8): 4}


def preprocess_masks(Y, L, min_counts_per_gene=20, min_counts_per_cell=100, remove_outlying_genes=True, nmads=10,
                     max_copy_number=6, remove_genes_same_copy_number=True, device=0, layout="row"):
    """Gene / cell retention masks of preprocess_for_clonealign() with the two O(N G) statistics taken on the device
    (ca_preprocess; R/preprocess.R:93-147).  Y [N, G] in float64/float32/int32/uint16/uint8 (other dtypes are converted
    to float64), L [G, C].  Returns (keep_gene bool[G], keep_cell bool[N], gene_sums[G], cell_sums[N])."""
    lib = load_library()
    Y = np.asarray(Y)
    if Y.dtype not in _NP_DTYPE:
        Y = Y.astype(np.float64)
    lay, order = _lay(layout)
    Y = np.require(Y, requirements=[order, "A"])
    L = np.require(np.asarray(L, dtype=np.float64), requirements=[order, "A"])
    N, G = Y.shape
    if L.shape[0] != G:
        raise ValueError("copy_number_data must have same number of genes (rows) as gene_expression_data")
    pp = CaPreprocessParams(float(min_counts_per_gene), float(min_counts_per_cell), int(bool(remove_outlying_genes)),
                            int(bool(remove_genes_same_copy_number)), float(nmads), float(max_copy_number))
    kg = np.zeros(G, dtype=np.uint8)
    kc = np.zeros(N, dtype=np.uint8)
    gs = np.zeros(G, dtype=np.float64)
    cs = np.zeros(N, dtype=np.float64)
    err = C.create_string_buffer(256)
    rc = lib.ca_preprocess(N, G, L.shape[1], lay, _NP_DTYPE[Y.dtype], 0, Y.ctypes.data_as(C.c_void_p),
                           L.ctypes.data_as(C.c_void_p), C.byref(pp), int(device), kg.ctypes.data_as(C.c_void_p),
                           kc.ctypes.data_as(C.c_void_p), gs.ctypes.data_as(C.c_void_p), cs.ctypes.data_as(C.c_void_p), err)
    if rc != CA_OK:
        raise EngineError(rc, err.value.decode() or "ca_preprocess")
    return kg.astype(bool), kc.astype(bool), gs, cs
