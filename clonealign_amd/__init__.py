"""clonealign_amd -- MI355X-native variational-inference engine for clonealign.

Drop-in for the hot path of kieranrcampbell/clonealign (``inference_tflow`` and its
callers ``clonealign`` / ``run_clonealign``): the TensorFlow ELBO loop is replaced by
hand-written HIP kernels for gfx950 behind the C ABI in ``include/clonealign_hip.h``.
"""
from .api import (ClonealignFit, ClonealignTracks, assign_cells, assign_cells_dm, assign_cells_marginal, assignment_support, clone_assignment, clone_evidence, clone_expression_profile, heldout_evidence, clone_loglik, clone_loglik_by_block, clone_loglik_dm, clone_pair_loglik,  # noqa: F401
                  clonealign, compute_ca_fit_mse, compute_correlations, detect_doublets, dosage_response, estimate_concentration, plot_clonealign, predictive_check, predictive_fit_mse, predictive_moments, project_cells, recompute_clone_assignment, refined_normal_cdf, run_clonealign,
                  simulate_counts, bootstrap_assignments, bootstrap_gene_weights, clone_loglik_reweighted, clone_separability, edgeworth_normal_cdf, merge_candidates, reads_needed,
                  copy_number_profile, suspect_copy_numbers, apply_copy_number_calls, clone_mixture, mixture_loglik, deconvolve_clones)
from .hostprep import inverse_softplus, safe_inverse_softplus, saturate, softplus  # noqa: F401
from .inference import inference_tflow  # noqa: F401
from .preprocess import preprocess_for_clonealign  # noqa: F401

__version__ = "0.1.0"
