/*
 * clonealign_hip.h -- C ABI of the MI355X (gfx950) variational-inference engine that
 * replaces the TensorFlow-backed ELBO loop of kieranrcampbell/clonealign.
 *
 * Boundary: the reference's only compute call site is
 *   inference_tflow()            R/inference-tflow.R:71-481
 * whose graph build (:240-346) and session loop (:351-457) talk to TensorFlow through
 * reticulate.  Each entry point below replaces one `sess$run(...)` granularity of that
 * loop, so an R shim can either keep the R-level loop verbatim or hand the whole loop to
 * ca_run().  Plain C types only: no R, Python, torch or HIP types cross this boundary.
 *
 * Conventions
 *   - every function returns CA_OK (0) or an error code; ca_last_error() gives the text.
 *   - matrices are passed in ONE layout per problem (`layout`): CA_COL_MAJOR is what R
 *     hands over (column-major, i.e. Y is gene-major in memory), CA_ROW_MAJOR is C/numpy.
 *   - `eps` arguments are host pointers to S*G float32 standard normals, sample-major
 *     (eps[s*G + g]): the noise of ONE `qmu$sample()` evaluation
 *     (R/inference-tflow.R:268-269).  Passing the stream explicitly is what makes results
 *     reproducible across engines; NULL selects the built-in Philox4x32-10 stream keyed by
 *     ca_options.seed (draw index kept in the handle).
 *   - handles are independent and re-entrant (no globals); one host thread per handle.
 */
#ifndef CLONEALIGN_HIP_H
#define CLONEALIGN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CA_ABI_VERSION 6

typedef struct ca_engine* ca_handle;

enum ca_status {
  CA_OK = 0,
  CA_ERR_INVALID = 1, /* bad argument / shape (the reference's stopifnot()/stop() cases) */
  CA_ERR_HIP = 2,     /* HIP runtime failure */
  CA_ERR_NOMEM = 3,
  CA_ERR_NAN = 4,     /* "Initial elbo is NA" (R/inference-tflow.R:374-376) or NaN in the window test (:414) */
  CA_ERR_COMM = 5,    /* RCCL / peer-to-peer transport failure */
  CA_ERR_STATE = 6,
  CA_INTERRUPTED = 7  /* ca_run_ex(): the poll callback asked to stop; trace and variables are those of the last completed iteration */
};

enum ca_dtype { CA_F64 = 0, CA_F32 = 1, CA_I32 = 2, CA_U16 = 3, CA_U8 = 4 };
enum ca_layout { CA_ROW_MAJOR = 0, CA_COL_MAJOR = 1 };
enum ca_ystore { CA_YSTORE_AUTO = 0, CA_YSTORE_F32 = 1, CA_YSTORE_U16 = 2, CA_YSTORE_U8 = 3 };

/* Inputs of one fit: what inference_tflow() has in hand at R/inference-tflow.R:236,
 * after its gene filter (:117-124), saturate (:142-144) and initialisation (:204-235). */
typedef struct ca_problem {
  int64_t N;           /* cells held by THIS process (a shard when world > 1) */
  int32_t G, C;        /* genes, clones */
  int32_t K, P, S;     /* latent dims (:136), covariates (:147-153), MC samples (:268) */
  int32_t layout;      /* ca_layout, applies to Y, L, psi0, X, extra_loglik and ca_get_param outputs */
  int32_t y_dtype;     /* ca_dtype of Y */
  int32_t y_on_device; /* nonzero: Y is a device pointer on ca_options.device */
  const void* Y;       /* N x G counts (:190,355) */
  const double* L;     /* G x C copy number (:191) */
  const double* psi0;  /* N x K  (:204-208, `pcs`)   -- may be NULL when K == 0 */
  const double* loc0;  /* G      (:262, safe_inverse_softplus(mu_guess)); NULL = the data_init_mu = TRUE guess of :220-235
                          computed from the resident matrix.  Sharded (world > 1, ABI 6): every rank keeps its cells' part of the
                          per-gene sums and the guess is completed over ALL cells by the first reduction of the transport the
                          engine is given (ca_comm_init / ca_p2p_commit / ca_set_host_allreduce), before any pass can run */
  const double* X;     /* N x P covariates or NULL (:147-153) */
  const double* extra_loglik; /* N x C additive log-lik (allele term, :302-304) or NULL */
  /* Optional row / column selection of Y, so that the masks of ca_preprocess() (R/preprocess.R:141-147 returns filtered
   * COPIES) or the gene filter of R/inference-tflow.R:117-124 never cut the matrix on the host: Y is then the RAW
   * N_src x G_src matrix and cell n / gene g of the problem is its row cell_index[n] / column gene_index[g] (0-based,
   * strictly increasing).  NULL = identity (then N_src / G_src are ignored).  L, psi0, loc0, X, extra_loglik are always
   * given for the SELECTED cells and genes. */
  int64_t N_src;
  int32_t G_src;
  const int64_t* cell_index;  /* N entries or NULL */
  const int32_t* gene_index;  /* G entries or NULL */
  /* ABI 6: leading dimension of Y in ELEMENTS, 0 = dense.  CA_COL_MAJOR: distance between two columns (>= the rows of the source
   * matrix); CA_ROW_MAJOR: distance between two rows (>= its columns).  With it a block of ROWS of a column-major matrix -- what a
   * shard of R's N x G matrix is -- is handed over in place (Y = &M[lo], y_ld = nrow(M)), and only that block crosses PCIe. */
  int64_t y_ld;
} ca_problem;

/* Decomposition variants (bits of ca_options.variant_off: a set bit switches the variant OFF; 0 = the measured defaults).
 * They exist so that every fallback stays under test and every choice can be re-measured. */
enum ca_variant {
  CA_VAR_FUSED = 1 << 0,      /* fused two-eps sweep (monitor pass i + forward half of train pass i+1) */
  CA_VAR_FWD_MFMA = 1 << 1,   /* forward contraction on the matrix cores */
  CA_VAR_FWD_CELL = 1 << 2,   /* forward sweep and cell epilogue in one kernel */
  CA_VAR_BWD_MFMA = 1 << 3,   /* backward contraction on the matrix cores */
  CA_VAR_TAIL_FUSE = 1 << 4,  /* O(K + C) bodies as extra blocks of other launches */
  CA_VAR_ASYNC_Y = 1 << 5,    /* count-matrix products on the side stream */
  CA_VAR_PRE = 1 << 6,        /* next pass's per-gene prologue on the per-cell Adam kernel */
  CA_VAR_PAIR_ELBO = 1 << 7,  /* final ELBOs two draws per sweep */
  CA_VAR_PREP_FAST = 1 << 8,  /* wave-per-cell fit-constant kernel for u8 storage */
  CA_VAR_UPDATE_MERGE = 1 << 9, /* the update half of a train pass of the loop as ONE launch (k_update_merged: per-gene step + next prologue + int8 images, psi,
                                  q(z) logits, chi / alpha), the exponent bound taken by the next forward sweep; off: k_final_gene + k_adam_cell */
  CA_VAR_P2P_RIDE = 1 << 16,  /* sharded over the peer-to-peer transport: the backward sweep's column sums, the stream's finishing sums and the pending monitor
                                 pass's psi.(YW) sum ride in the sweep's and the all-reduce's launches (4 launches per iteration); off: k_yfinish + k_colsum launches */
  CA_VAR_RUN_GATE = 1 << 17,  /* ca_run: the update half of the next train pass is queued before the host has seen the ELBO its stop rule needs and waits ON THE
                                 DEVICE for the host's go / stop word (no launch latency between the decision and the update) -- for gate_timeout_us at most, then
                                 it gives up, stores nothing and is queued again after the decision; off: always queued after the decision */
  CA_VAR_S2_FUSE = 1 << 18,   /* mc_samples = 2: the monitor pass's two samples and the next train pass's two samples in ONE forward sweep (two operand sets,
                                 four draws on one exp per (cell, gene)); off: a sweep per pass */
  CA_VAR_FWD_BAL = 1 << 19,   /* small problems (one to six 16-cell tiles per CU): ONE eight-wave forward-sweep block per CU, the left-over tiles spread gene-wise over
                                 the blocks with their partial Z exchanged through tagged words (k_fwd_bal_ys, ca_fwdbal.hip.h): every SIMD holds two waves with equal
                                 work; off: 16- / 32-cell four-wave blocks, as many as the cells need */
  CA_VAR_BWD_TL3 = 1 << 20,   /* small problems (up to 18 432 cells): the matrix-core backward sweep takes three gene tiles per wave instead of four -- more and
                                 shorter wave jobs; off: four at every size */
  CA_VAR_SERIES = 1 << 21,    /* ABI 6: large problems with a rank-one exponent (K + P = 1, one MC sample, 3..8 clones, 1-byte storage; where G >= 2000 + 2.5e7 / N -- the round's first form: from 32k cells and 1.4e8
                                 counts): the loop's contraction in its SERIES form (ca_poly.hip, see CA_VARX_SERIES) -- moments over gene bins instead of the
                                 cells x genes sweeps; off: the matrix-core sweeps at every size */
  CA_VAR_P2P = 1 << 10,       /* one-shot peer-to-peer all-reduce (else ncclAllReduce) after ca_comm_init() */
  CA_VAR_FOLD_GSUM = 1 << 11, /* small problems: backward-sweep partials summed inside the per-gene kernel (else a k_colsum launch) */
  CA_VAR_Y_RIDE = 1 << 12,    /* the Y stream's blocks ride on the forward sweep's launch (else side stream / in line) */
  CA_VAR_Y_MFMA1 = 1 << 14,   /* both count-matrix products on the int8 matrix cores from ONE tiled copy of the 1-byte matrix, the column products
                                 through the transposing LDS read ds_read_b64_tr_b8 (ca_ymfma.hip.h; K = 1): the default since round 3, when its
                                 blocks ride on the forward sweep as long-lived stream blocks and its quantiser on the per-cell Adam kernel.
                                 Off: the vector stream (k_ypass / k_fwd_cell_mix_y) */
  CA_VAR_YFIN_RIDE = 1 << 15, /* the riding int8 stream's finishing sums (Y^T psi column sums, YW and the psi.(YW) partials) as extra blocks of the
                                 backward sweep's launch; the pending monitor pass's ELBO is then assembled one kernel later (per-gene kernel).
                                 Off: a finisher launch (k_yfinish) between the two sweeps */
  CA_VAR_Y4 = 1 << 22,        /* the one-copy stream's loop image at 4 bits per count (min(y, 15) in a nibble, the counts from 15 up as their exact excess in
                                 an escape list bucketed by the stream's own units): half the bytes per pass, the same integer sums; picked where the escapes
                                 are at most 1 in 64 counts (CA_VARX_Y4 forces it).  Off: the 1-byte loop image */
  CA_VAR_MOM_RIDE = 1 << 23,  /* the series form's forward moments (bin geometry, per-group partials, their fixed-order sums) as the first blocks of its count-matrix
                                 stream's launch instead of two launches in front of it: two launches and their boundaries less per iteration, the same additions
                                 in the same order; on wherever the series form runs its stream in line.  Off: k_poly_B + k_poly_red, then the stream */
  CA_VAR_CELL_LEAN = 1 << 24, /* the series form's cell launch with nothing on a pass's chain of latencies that the result does not need: no global load inside a pass
                                 but the prefetch of the next one (no read of the zero exponent bound; c_n and psi come with the prefetch), the 4- and 8-lane reductions
                                 through DPP moves instead of the LDS crossbar, the powers of x without a branch per step; the same additions in the same order; on
                                 wherever the series form runs.  Off: the launch as it was (k_poly_cell<CP, false>) */
  CA_VAR_MOM_LAST = 1 << 25,  /* the moment role of CA_VAR_MOM_RIDE BEHIND the stream's blocks in the launch's grid instead of in front of them, where a host rule says
                                 that this hides it (the stream's blocks and the role exceed one round of block slots, every XCD keeps a free slot, the role's chain
                                 in the free slots fits under the stream's time): every stream block is resident from the start and none waits for a block of the
                                 role to leave.  Scheduling only: the same bits.  Off: the role in front, block for block the launch as it was (CA_VARX_MOM_LAST
                                 forces the order wherever the moments ride) */
  CA_VAR_CELL_MFMA = 1 << 26, /* the series form's cell launch gathers the backward moments of its register bins as a matrix product per wave (v_mfma_f64_16x16x4_f64
                                 over the wave's own cells, accumulators kept over the block's passes, the four waves' tiles added in wave order at the block's end)
                                 instead of a 32-step chain on 176 threads between two block barriers: with at most four bins a pass has no block barrier left.  The
                                 same sums in another, fixed association: fp64 rounding apart, the same bits from run to run; on wherever the series form runs.
                                 Off: the thread-owned chain (k_poly_cell<CP, LEAN, false>), the launch as it was */
  CA_VAR_Y2 = 1 << 27,        /* the series form's own count-matrix stream launch reads a third loop image in which the genes of each 512-gene segment are ordered by how
                                 often they reach 3 and the first N2 64-gene blocks of every segment hold min(y, 3) in 2 bits (the counts from 3 up in its own escape
                                 list), the others 4 bits as before: fewer bytes per pass, the same integer sums.  Picked where the 4-bit image is, the matrix is
                                 large enough for the launch to follow its bytes, and N2 = 6 or 5 keeps the escapes at 1 in 256 counts (CA_VARX_Y2 forces N2 = 6).
                                 Off: the 4-bit image's launch as it was */
  CA_VAR_GENE_RIDE = 1 << 28, /* the series form's way back from its cell launch: the count-matrix stream's column sums, which nobody reads before the update, leave the
                                 cell launch (whose extra blocks can only start in slots its cell blocks have left), and an unsharded pass runs the reduction of the
                                 backward moments, the per-gene pass, the pending monitor pass's tail and those column sums as ONE launch, the moment table handed over
                                 inside it through tagged words (ca_polygene.hip.h) -- a launch and a kernel boundary less per iteration; a cell-sharded fit keeps
                                 reduction and per-gene pass apart (its collective sits between them) and carries the column sums on the reduction launch.  The same
                                 additions in the same order: the same bits.  Off: cell launch, k_poly_red and k_poly_gene as they were */
  CA_VAR_CELL_EDGE = 1 << 29, /* the series form's cell launch (lean passes, MFMA gather) with what stands around its passes off their critical path: every load of a
                                 block's head (first prefetch, bin geometry, the bins' tables, alpha) issued before the first wait, and the block's end as one parking
                                 step -- every wave leaves its sums and tiles in the passes' idle LDS arrays at once, and after one barrier the finishing adds are
                                 shared between the waves.  Every sum keeps its operands and its order: the same bits.  Off: the launch as it was
                                 (k_poly_cell<CP, true, true, false>) */
  CA_VAR_RIDE_SEQ = 1 << 13 /* (no effect: it was the off-switch of CA_VARX_RIDE_SEQ, whose code is deleted; the bit keeps its value, accepted and ignored) */
};
/* Opt-in variants (bits of ca_options.variant_on).  Those marked RETIRED were measured slower than what ships (rounds 2-5: DESIGN_HISTORY.md, profiles/) and their
 * code has been deleted; the constants keep their values and ca_create returns CA_ERR_INVALID for them, in every build. */
enum ca_variant_on {
  CA_VARX_Y_MFMA2 = 1 << 0,   /* RETIRED.  count-matrix products on the int8 matrix cores from TWO tiled copies (cell-tiled for Y.W,
                                 gene-tiled for Y^T.psi): 6.0 TB/s per stream against 4.7 for k_ypass, but twice the bytes per iteration */
  CA_VARX_Y_MFMA1 = 1 << 2,   /* (round 2's opt-in for what is now the default, CA_VAR_Y_MFMA1; accepted and ignored) */
  CA_VARX_FOLD_ALWAYS = 1 << 3, /* backward-sweep partials summed inside the per-gene kernel at every size (default: up to 32k cells) */
  CA_VARX_RIDE_SEQ = 1 << 4,  /* RETIRED.  riding Y stream fused in sequence: every forward-sweep block also streamed one unit of the count matrix,
                                 before or after its sweep, instead of separate stream blocks in the same grid */
  CA_VARX_P2P_SAME_DEVICE = 1 << 5, /* test rigs only: let ca_p2p_connect map a peer handle of the SAME process on the SAME device (refused
                                 otherwise: device-wide synchronising runtime calls of one handle would wait on the other's all-reduce) */
  CA_VARX_RUN_FWD = 1 << 6,   /* ca_run with the gated update: the forward sweep behind it is queued before the host's decision as well (its blocks return at
                                 their first instruction on "stop").  OPT-IN, and only for a process whose ONLY user of the GPU runtime is this engine's thread:
                                 the sweep is queued while the gated update may already be waiting for the host, and a runtime call made in that window can block
                                 behind another thread that holds a runtime lock while IT waits for the GPU (two engines of one process on one device did exactly
                                 that: the update then gives up after its 10 s and ca_run returns CA_ERR_STATE).  Worth about 1 us per iteration. */
  CA_VARX_BAL_TILES = 1 << 7, /* RETIRED.  balanced forward sweep of small problems (CA_VAR_FWD_BAL): a single-tile block of its own per left-over tile behind the
                                 sweep blocks, no exchange, instead of the left-over tiles cut gene-wise into chunks that the sweep blocks sweep beside their own
                                 tiles.  Level at few left-over tiles, slower at many */
  CA_VARX_SERIES = 1 << 8,    /* ABI 6: force the series form (CA_VAR_SERIES) at ANY size.  The form: where the exponent is rank one -- K + P = 1, one MC sample, 3..8
                                 clones: Z_nc = sum_g M_gc exp(x_n v_g) is one function of x per clone; genes binned by v, a 20-term expansion per bin (argument <= 2,
                                 float64): moments over genes, evaluation over cells, the same form on the way back.  No cells x genes sweep: O(N nb R C + G R C)
                                 instead of O(N G C) per pass; the cell epilogue is the sweep's.  Other shapes keep the matrix-core sweeps */
  CA_VARX_Y4 = 1 << 9,        /* the 4-bit loop image (CA_VAR_Y4) at any escape fraction */
  CA_VARX_MOM_LAST = 1 << 10, /* the moment role behind the stream's blocks (CA_VAR_MOM_LAST) wherever the moments ride, whatever the rule says (the bits are the same) */
  CA_VARX_Y2 = 1 << 11,       /* the 2-bit / 4-bit image (CA_VAR_Y2) wherever the series form streams the 4-bit image, at any size and escape fraction, N2 = 6 */
  CA_VARX_ASYNC_SMALL = 1 << 1 /* side stream also below 4e7 counts (small shards run the Y stream in line: the two cross-stream
                                 events cost more than the overlap returns there) */
};
#define CA_OPT_VERBOSE 0x80000000u /* in variant_off: print the decomposition picks to stderr */
/* decomposition parameters the heuristics pick; a non-zero ca_options.tune[id] overrides (CA_TUNE_FC_NBIG: -1 = one block size) */
enum ca_tune_id {
  CA_TUNE_GSPLIT = 0, CA_TUNE_FSPLIT = 1, CA_TUNE_FC_TL = 2, CA_TUNE_FC_NBIG = 3, CA_TUNE_CSPLIT = 4, CA_TUNE_CSPLIT_M = 5,
  CA_TUNE_TR = 6, CA_TUNE_RG = 7, CA_TUNE_COUNT = 8
};

typedef struct ca_options {
  double learning_rate;             /* :75,345 */
  double beta1, beta2, adam_eps;    /* tf.train.AdamOptimizer defaults 0.9, 0.999, 1e-8 */
  uint64_t seed;                    /* key of the built-in eps stream */
  int32_t device;                   /* HIP device ordinal */
  int32_t y_storage;                /* ca_ystore: on-device width of the count matrix */
  int32_t rank, world;              /* cell-sharded data parallel: shard `rank` of `world` */
  int32_t profile;                  /* bits 0..4: bitmask over ca_kernel_id, time those kernel classes with HIP events; bits 8..15: sampling
                                     * stride - 1 (0 = every launch; an event pair costs the stream 5-6 us, so live measurements sample) */
  uint32_t variant_off;             /* ca_variant bits to switch off (| CA_OPT_VERBOSE); 0 = defaults */
  int32_t tune[8];                  /* ca_tune_id overrides, 0 = heuristic */
  uint32_t variant_on;              /* ca_variant_on bits to switch on; 0 = defaults */
  int32_t ride_pattern;             /* dispatch order of the merged forward launch (sweep blocks + Y-stream blocks in one grid).  0 = default:
                                     * one LONG-LIVED stream block per CU leads the grid, each walks through every n-th unit of the count matrix
                                     * (from two units per CU up; below that the 2:1 interleave).  < 0: that many long-lived stream blocks.
                                     * > 0: (a << 8) | b = a sweep blocks, then b single-unit stream blocks, ...; periods that divide 8 put the
                                     * two kinds on disjoint XCDs.  Results do not depend on it (tests/test_gpu_parity.py) */
  int32_t comm_timeout_ms;          /* peer-to-peer all-reduce: how long a rank waits on the device for its peers' data before the call
                                     * gives up and the engine reports CA_ERR_COMM (0 = 10 000 ms) */
  int32_t gate_timeout_us;          /* ca_run with the gated update (CA_VAR_RUN_GATE): how long the queued update's relay block polls for the host's
                                     * go / stop word before the launch gives up -- it then stores nothing, the device goes idle, and the host queues
                                     * the update again after its decision (0 = 1000 us).  Not an error and not a result: only who waits for whom */
  int32_t reserved[2];              /* lab knobs of the series form: [0] cell blocks per CU (0 = 2), [1] = 1: its count-matrix stream on the side stream (measured slower), 7 / 8: with CA_VAR_GENE_RIDE the stream's column sums stay behind the cell launch's blocks / go with the reduction, whatever the size rule says (A/B runs; the same bits) */
} ca_options;
/* (The library reads no tuning from the process environment.  Only the timing-lab build, -DCA_LAB -- never the product's .so, its
 *  ca_build_id() starts with "lab-" -- accepts the same switches as CA_* variables, and only when CLONEALIGN_DEBUG_ENV is set.) */

typedef struct ca_info {
  int64_t N;
  int32_t G, C, K, P, S;
  int32_t y_storage;         /* ca_ystore actually used */
  int32_t y_bytes_per_elem;
  int64_t y_device_bytes;    /* resident size of the count matrix */
  int64_t device_bytes;      /* total device allocation of this handle */
  int32_t gsplit, csplit;    /* gene / cell splits of the forward / backward sweeps */
  int32_t n_cu;
  int32_t fused_sweep;       /* 1: ca_run/ca_iterate fuse monitor pass i with the forward half of train pass i+1 */
  int32_t fwd_mfma;          /* 1: the fused sweep's forward contraction runs on the matrix cores (k_fwd_mfma) */
  int32_t bwd_mfma;          /* 1: the backward sweep's t = coef.L contraction runs on the matrix cores (k_bwd_mfma) */
  int32_t fsplit;            /* gene slices of the matrix-core forward sweep */
  int32_t fwd_cell;          /* 1: forward sweep and cell epilogue of the fused pass are ONE kernel (k_fwd_cell) */
  int32_t y_mfma;            /* the loop's count-matrix products on the int8 matrix cores: 0 no (k_ypass), 2 from one tiled copy (1, two tiled copies, is no longer reported: CA_VARX_Y_MFMA2 is retired) */
  int32_t transport;         /* 0 none, 1 RCCL all-reduce, 2 host callback, 3 one-shot peer-to-peer (ca_transport) */
  int32_t y_ride;            /* 1: the Y stream's blocks ride on the fused forward sweep's launch (k_fwd_cell_mix_y): no launch of its own */
  int64_t red_n;             /* doubles all-reduced per train pass (= sharding.reduce_plan(...)["total"]) */
  /* ABI 4: which decomposition the shape selected (the tests assert that their shapes cross every threshold) */
  int32_t fwd_block_cells;   /* cells per block of the fused forward sweep: 16, 32 or 96 (0: no fused forward sweep) */
  int32_t fwd_blocks_big;    /* > 0: mixed launch, that many blocks of fwd_block_cells cells, the rest 32-cell blocks */
  int32_t fold_gsum;         /* 1: the backward sweep's per-gene partials are summed inside the per-gene kernel (unsharded small problems) */
  int32_t yfin_split;        /* 1: the Y stream's finishing step is split between the forward and backward launches */
  int32_t update_merge;      /* 1: the loop's update half is one launch (CA_VAR_UPDATE_MERGE) */
  int32_t fwd_balanced;      /* > 0: the fused forward sweep is the balanced small-problem form (CA_VAR_FWD_BAL), that many tiles per block */
  int32_t fwd_series;        /* ABI 6: 1: the loop's contraction takes its series form (CA_VAR_SERIES / CA_VARX_SERIES, ca_poly.hip) wherever the exponent range allows */
  int32_t y_stream_bits;     /* bits per count of the one-copy stream's loop image: 8, or 4 (CA_VAR_Y4); 0 where there is no loop image */
  int64_t series_passes;     /* fused passes of this engine that ran in the series form ... */
  int64_t series_fallbacks;  /* ... and those the look ahead at the exponent range (max|psi| (max W - min W), plus what the Adam steps since can add) gave to the sweeps */
  int32_t mom_ride;          /* 1: the series form's forward moments ride on its count-matrix stream's launch (CA_VAR_MOM_RIDE) */
  int32_t cell_lean;         /* 1: the series form's cell launch runs its lean passes (CA_VAR_CELL_LEAN) */
  int32_t mom_last;          /* 1: the riding moment role sits behind the stream's blocks in the launch's grid (CA_VAR_MOM_LAST / CA_VARX_MOM_LAST); 0: in front */
  int32_t mom_free_slots;    /* block slots of the stream's launch (occupancy x compute units, asked of the runtime) that its own blocks leave free: what the rule saw; 0 where no moments ride */
  int32_t cell_mfma;         /* 1: the series form's cell launch gathers its backward moments by fp64 MFMA per wave (CA_VAR_CELL_MFMA) */
  int32_t y_stream_n2;       /* > 0: the series form's own stream launch reads the 2-bit / 4-bit image (CA_VAR_Y2): that many of a segment's eight 64-gene blocks hold 2 bits per
                                count, the others y_stream_bits (which stays the width of the wide blocks); 0: no 2-bit blocks */
  int64_t y_stream_esc;      /* entries of the escape list the series form's own stream launch reads (the 2-bit / 4-bit image's where y_stream_n2 > 0, else the 4-bit image's; 0 at 8 bits) */
  int64_t y_stream_bytes;    /* bytes that launch reads per pass: its image plus its escape list */
  int32_t gene_ride;         /* 1: a series pass of this engine runs reduction, per-gene pass and the stream's column sums as one launch (CA_VAR_GENE_RIDE); 0: as launches
                                of their own (the switch off, no series form, or a cell-sharded fit) */
  int32_t cell_edge;         /* 1: the series form's cell launch issues its head's loads at once and ends its blocks in one parking step (CA_VAR_CELL_EDGE) */
} ca_info;
enum ca_transport { CA_TRANSPORT_NONE = 0, CA_TRANSPORT_RCCL = 1, CA_TRANSPORT_HOST = 2, CA_TRANSPORT_P2P = 3 };

/* kernel classes reported by ca_get_kernel_times() */
enum ca_kernel_id {
  CA_KERNEL_FWD = 0,    /* Z = E.M sweep            (R/inference-tflow.R:278-292) */
  CA_KERNEL_BWD = 1,    /* reverse sweep of the same contraction (autodiff of :288-296) */
  CA_KERNEL_YPASS = 2,  /* Y.W and Y^T.psi stream   (the y*log p part of :294-296) */
  CA_KERNEL_CELL = 3,   /* per-cell epilogue: log-lik, softmax, ELBO partials (:294-308,332-333) */
  CA_KERNEL_OTHER = 4,  /* per-gene terms, reductions, Adam (:311-336,345-346) */
  CA_KERNEL_COUNT = 5
};

int ca_abi_version(void);
const char* ca_build_id(void); /* first 16 hex digits of the SHA-1 over the library's sources, as built */
/* Number of HIP devices this library's runtime sees (0 and CA_ERR_HIP when there is none).  Also initialises the runtime: a host
 * that loads a second HIP runtime into the process (PyTorch bundles its own) should call this right after loading the library,
 * so that the load order and the initialisation order agree (the runtime initialised second after being loaded first sees
 * "no ROCm-capable device"). */
int ca_device_count(int32_t* n);
int ca_default_options(ca_options* opts);

/* Build the engine: upload Y/L/init, precompute the fit constants (lgamma terms,
 * A = Y.log L, column sums), zero-initialise the variables as :240-272 does.
 * Replaces graph construction + `sess$run(init)` (:240-353). */
int ca_create(const ca_problem* problem, const ca_options* opts, ca_handle* out);

/* Sparse count matrices (additions to ABI 6): the compressed form of Y -- scipy's csr / csc matrices, R's dgCMatrix -- goes to the
 * device as it is (no N x G copy on the host or in a staging buffer), is validated and scanned there, and is expanded into the same
 * resident [N][Gp] matrix (and u8 overflow list) ca_create builds from the dense form: every fit on it is the dense fit, bit for bit.
 * Implicit zeros are zeros; the storage pick (ca_options.y_storage, AUTO) is taken over the SELECTED counts exactly as for a dense Y. */
enum ca_sparse_kind { CA_SPARSE_CSR = 0,   /* one run per cell: ptr has N_src + 1 entries, idx are gene indices
                                              (scipy csr of cells x genes; the CSC dgCMatrix of a genes x cells assay) */
                      CA_SPARSE_CSC = 1 }; /* one run per gene: ptr has G_src + 1 entries, idx are cell indices (dgCMatrix / scipy csc of cells x genes) */
typedef struct ca_sparse {
  int32_t kind;         /* ca_sparse_kind */
  int32_t val_dtype;    /* ca_dtype of val: CA_F64 (R's @x), CA_F32, CA_I32, CA_U16, CA_U8 */
  int32_t index_bytes;  /* 4 or 8: width of ptr AND idx (R: 4; scipy: 4 or 8; torch: 8) */
  int32_t on_device;    /* ptr / idx / val are device pointers on ca_options.device */
  int64_t nnz;
  const void* ptr;
  const void* idx;      /* canonical: strictly increasing within each run; explicit zeros allowed */
  const void* val;
} ca_sparse;
/* ca_create with the count matrix in compressed form.  problem->Y must be NULL; y_dtype, y_on_device and y_ld are ignored; layout
 * still applies to L, psi0, X, extra_loglik and the outputs.  The matrix is N_src x G_src with a selection (cell_index / gene_index,
 * as for ca_create), else N x G.  Canonical form, checked on the device (CA_ERR_INVALID with a message otherwise): ptr[0] = 0,
 * ptr never decreases, ptr[last] = nnz, every idx in range and strictly increasing within its run.  Host arrays go up in their own
 * dtype (float64 values narrowed to float32 on the way, as a dense float64 Y is); peak device memory while ingesting is the resident
 * matrix plus the compressed arrays (plus their CSR transpose for CSC).  The arrays are read during the call only. */
int ca_create_sparse(const ca_problem* problem, const ca_sparse* y, const ca_options* opts, ca_handle* out);
int ca_destroy(ca_handle h);
const char* ca_last_error(ca_handle h); /* h may be NULL: error of the last failed ca_create on this thread */
int ca_get_info(ca_handle h, ca_info* info);
int ca_synchronize(ca_handle h);
/* *busy = 1 while work queued on the engine's stream has not completed, else 0; never blocks, never changes anything (a poll hook can
 * watch the device drain while it holds the loop up). */
int ca_stream_busy(ca_handle h, int32_t* busy);
/* Read-only, for tests and diagnostics: what the last launch of the one-copy count-matrix stream (K = 1; ca_info.y_mfma = 2) left, before its finisher sums it.
 * CA_ERR_INVALID on an engine without that stream, CA_ERR_STATE before its first launch (ca_elbo / ca_gradients / a loop call makes one).  Changes no result; a
 * launch still running on the engine's side stream is waited for.  dims = {nseg, N, nrg, Gp, RS, images_current}, N64 = N rounded up to 64; every other pointer may be NULL (call once for dims).
 *   yw_part [nseg][N]  float: the segment's (512 genes) share of (Y W)_n, = (float)(v 2^-exps[0]), v = sum_g min(y_ng, 255) fix(W_g) as an exact integer
 *   yt_part [nrg][Gp]  float: the row group's (4 strips of RS cells) share of (Y^T psi)_g, = (float)(v 2^-exps[1]), v = sum_n min(y_ng, 255) fix(psi_n)
 *                      (counts above 255 keep 255 in the resident matrix; their excess goes through the overflow list, outside these slabs)
 *   exps    [2]        the fixed-point exponents that launch read (W, psi)
 *   w_fix [Gp], p_fix [N64]  the fixed-point values in the parameter images NOW, fix(x) = rint(x 2^exp), zero past G and N.  images_current = 1: they are
 *                      the ones that launch read (after ca_gradients / ca_elbo); 0: the parameters have moved since (after ca_step / ca_iterate / ca_run: the
 *                      loop's update quantises the new state), and fix() of the state before the step reproduces them from exps. */
int ca_ystream_parts(ca_handle h, int64_t dims[6], float* yw_part, float* yt_part, int32_t exps[2], int32_t* w_fix, int32_t* p_fix);

/* cell-sharded multi-GPU (one process per GPU): RCCL communicator over xGMI.
 * Rank 0 calls ca_comm_unique_id() and distributes the 128 bytes out of band. */
int ca_comm_unique_id(char id[128]);
int ca_comm_init(ca_handle h, const char id[128]);
/* One-shot peer-to-peer all-reduce over xGMI: the per-iteration payload is ~120 KB, i.e. latency-bound, so
 * instead of a ring every rank WRITES its summands into an inbox slab of every peer (IPC-mapped device memory) and adds the W
 * inboxes of its own slab in rank order 0..W-1 -- the same additions in the same order on every rank, so the replicas stay
 * bit-identical, in one kernel on the engine's stream, no host round trip.  Since round 4 every 8-byte store carries half a double
 * and the call's 32-bit tag: a summand is complete when it can be READ complete -- no fence, no flag, no counter (k_p2p_allreduce).  Setup: every rank exports a handle, the caller exchanges them out of band (like the RCCL id: torch.distributed /
 * MPI all-gather), every rank connects.  Needs peer access between the devices (same node); ranks may share a device. */
#define CA_P2P_HANDLE_BYTES 128
/* Setup is two-phase so that a one-sided failure cannot leave the other ranks waiting on the device:
 *   1. every rank: ca_p2p_export (allocates the slab in FINE-GRAINED device memory -- CA_ERR_COMM when that is unavailable, never
 *      a coarse-grained fallback -- and returns the handle); the caller all-gathers the handles out of band;
 *   2. every rank: ca_p2p_connect (maps the peers' slabs: IPC handles of other processes, the slab's own address for handles of
 *      the SAME process -- one host process may drive several devices, one handle per DEVICE on one host thread each; peer access
 *      is enabled between different devices; two handles of one process on one device are refused).  Launches nothing and waits
 *      for nobody;
 *   3. the caller agrees over its control plane whether step 2 succeeded on EVERY rank, then every rank calls
 *      ca_p2p_commit(h, all_ok): 1 makes the transport the engine's all-reduce and reduces the setup sums (the first call that
 *      waits for peers); 0 drops the mappings (next: ca_comm_init, or a host callback).
 * The device-side wait for the peers' data is bounded (ca_options.comm_timeout_ms): when it runs out the call gives up (its buffer
 * is then partly summed), every later all-reduce on this engine returns at once, and the next API call that synchronises returns CA_ERR_COMM.
 * The engine is then dead: destroy it (a fresh process is the recovery).  Calls that reduce are collective: every rank must make
 * the same sequence of ca_* calls, and a ca_run_ex poll hook must take the same decision on every rank. */
int ca_p2p_export(ca_handle h, char handle[CA_P2P_HANDLE_BYTES]);
int ca_p2p_connect(ca_handle h, const char* handles /* world x CA_P2P_HANDLE_BYTES, in rank order */);
int ca_p2p_commit(ca_handle h, int32_t all_ranks_ok);
/* us per all-reduce of n_doubles doubles on one device transport (CA_TRANSPORT_P2P or CA_TRANSPORT_RCCL) of this engine, n_calls
 * back to back on the engine's stream between two HIP events; collective.  bench.py reports it beside the iteration time. */
int ca_comm_benchmark(ca_handle h, int32_t transport, int32_t n_calls, int64_t n_doubles, double* us_per_call);
/* Known-answer test of the engine's ACTIVE all-reduce (whatever ca_info.transport says): n_rounds all-reduces whose summands are
 * (rank + 1) * pattern(i, round) + round / 2 -- every partial sum is an integer or a half, exact in a double in any order -- checked on the host
 * against W (W + 1) / 2 * pattern + W * round / 2.  Call sizes alternate as the loop's do -- n_doubles (the train pass's payload), min(n_doubles, 11)
 * (a monitor pass's), and a vector longer than the peer-to-peer inbox (several pieces per call) -- in bursts of eight back-to-back calls with
 * no host synchronisation between them (both inbox parities and the sequence tags at the loop's own pace); on the peer-to-peer transport
 * four calls of the RIDE form follow (slab fold + block-partial sum inside the all-reduce's launch, checked against the same sums made on the
 * host).  *n_bad = entries that came back wrong (0 = the transport adds what it should).  Collective.  The first time a transport runs on
 * hardware it has never run on (peer-to-peer across xGMI), this is what a launcher asks before it trusts it (bench.py: 48 rounds). */
int ca_comm_selftest(ca_handle h, int32_t n_rounds, int64_t n_doubles, int64_t* n_bad);
/* Alternative transport for world > 1 (MPI, gloo, tests): the engine hands the summand buffer to the
 * host callback, which must replace buf[0..n) by its sum over all ranks (same order on every rank)
 * and return 0.  Slower than RCCL (one device<->host round trip per reduction); same results. */
typedef int (*ca_host_allreduce_fn)(void* user, double* buf, int64_t n);
int ca_set_host_allreduce(ca_handle h, ca_host_allreduce_fn fn, void* user);

/* `sess$run(gamma_init)` + `sess$run(init_gamma)`   (:338-342,368-369) */
int ca_gamma_init(ca_handle h, const float* eps);
/* `sess$run(elbo)`                                   (:336,372,403,448) */
int ca_elbo(ca_handle h, const float* eps, double* elbo);
/* the three summands of :336 -- EE_p_y, E_log_p_p, E_log_q */
int ca_elbo_terms(ca_handle h, const float* eps, double terms[3]);
/* `sess$run(train)`: forward + backward + TF1 Adam on all variables (:345-346,401) */
int ca_step(ca_handle h, const float* eps);
/* gradients of the ELBO without the Adam update (for parity checks); fetch with ca_get_gradient */
int ca_gradients(ca_handle h, const float* eps, double* elbo);

/* The whole session loop :368-417: gamma init (draw 0), initial ELBO (draw 1), then up to
 * max_iter iterations of {train, monitor} with the 10-long mean |relative change| < rel_tol
 * stop rule.  eps_stream: n_draws*S*G floats consumed in order (needs >= 2 + 2*max_iter
 * draws) or NULL for the built-in stream.  elbo_trace receives 1 + iterations values. */
int ca_run(ca_handle h, int32_t max_iter, double rel_tol, const float* eps_stream, int64_t n_draws,
           double* elbo_trace, int32_t* n_elbo);
/* The same loop with a host callback between iterations -- the reference's loop is R-level and can be interrupted or
 * observed every iteration (R/inference-tflow.R:394-417, progress bar :395-399).  poll(user, i, elbo_i) is called once
 * per ELBO value as the host learns it (i = 0 for the initial ELBO of :372, then 1, 2, ...), from the calling thread,
 * while the GPU already works on the backward sweep of the next train pass.  A non-zero return stops the loop exactly
 * like the convergence test does: the variables are those after iteration i, the trace has i + 1 values, and the call
 * returns CA_INTERRUPTED.  An R shim calls R_CheckUserInterrupt() through R_ToplevelExec() here. */
/* What a hook may do (ABI 5).  It may take as long as it likes -- a progress bar, a debugger, a sleep: the update the engine had queued
 * ahead of the hook's decision waits on the device for ca_options.gate_timeout_us at most, then gives up without storing anything and is
 * queued again after the hook returns; the fit is the same bit for bit, only that iteration loses the overlap.  It may call the read-only
 * entry points on this handle -- ca_get_param, ca_get_gradient, ca_get_info, ca_synchronize, ca_get_kernel_times, ca_stream_busy -- and sees
 * the variables after iteration `iter` (the first such call ends the queued update's wait the same way).  Every call that changes the
 * engine's state (ca_step, ca_set_param, ca_reinit, ca_run, ca_destroy, the ca_comm_* family ...) returns CA_ERR_STATE from inside a hook.
 * Sharded fits: the hook must take the same decision on every rank. */
typedef int (*ca_poll_fn)(void* user, int32_t iter, double elbo);
int ca_run_ex(ca_handle h, int32_t max_iter, double rel_tol, const float* eps_stream, int64_t n_draws,
              double* elbo_trace, int32_t* n_elbo, ca_poll_fn poll, void* user);
/* n_iter iterations of {train, monitor} with no convergence test and no host sync inside
 * (the benchmark "step"); last_elbo may be NULL.  eps_stream: 2 n_iter draws consumed in order.  ABI 6: given ONE MORE draw (2 n_iter + 1), the
 * call's last sweep also makes the forward half of the first train pass of the NEXT ca_iterate call with it; that call picks it up when its own
 * first draw is that draw bit for bit (else it is dropped, nothing else changes): back-to-back calls then run n_iter sweeps each instead of
 * n_iter + 1.  The variables, the ELBOs and the number of draws CONSUMED (2 n_iter) are the same either way; the built-in stream (NULL) looks
 * one draw ahead by itself.  Any other call in between drops the carried half. */
int ca_iterate(ca_handle h, int32_t n_iter, const float* eps_stream, int64_t n_draws, double* last_elbo);
/* `replicate(20, sess$run(elbo))` (:447-454): values[n_rep], mean and sample sd */
int ca_final_elbo(ca_handle h, int32_t n_rep, const float* eps_stream, int64_t n_draws, double* values,
                  double* mean, double* sd);

/* psi initialisation on the device (R/inference-tflow.R:204-208): the first K principal components of the standardised
 * log2(Y + 1) matrix (prcomp(center = TRUE, scale = TRUE)), each scaled to unit variance (scale()), plus `noise`
 * (N x K in the problem's layout, the reference's rnorm(.., 0, 0.05), or NULL).  Blocked subspace iteration on the resident
 * count matrix (two passes over Y per iteration, K + 4 vectors); component signs are fixed by making the loading of largest
 * magnitude positive (prcomp's own signs are LAPACK's and arbitrary).  Overwrites psi; pcs_out (N x K) may be NULL. */
int ca_init_psi_pca(ca_handle h, const double* noise, int32_t n_iter, uint64_t seed, double* pcs_out);

/* Per-gene sums behind compute_correlations() (R/clonealign.R:318-334), one pass over the resident counts instead of
 * shipping Y back: clone_of_cell[n] in [0, C) or -1 ("unassigned", dropped at :319-320).
 *   T[g][c] = sum over cells assigned to clone c of y_ng      (G x C, problem layout)
 *   Syy[g]  = sum over assigned cells of y_ng^2
 * Both are float64 sums in a fixed order (u8 overflow entries with their true values): T is exact for integer counts in every storage
 * while a total stays below 2^53, Syy good to float64 rounding -- n Syy - (sum_c T)^2 of the correlation cancels most of its digits.
 * Pearson's r of (copy number of the assigned clone, counts) follows from T, Syy and the clone sizes on the host. */
int ca_clone_gene_sums(ca_handle h, const int32_t* clone_of_cell, double* T, double* Syy);

/* Squared error of a fit, compute_ca_fit_mse() (R/clonealign.R:415-434), in ONE sweep over the resident counts (any storage; the
 * matrix is not shipped back and no N x G array is made): clone_of_cell[n] in [0, C), or -1 for a cell that is skipped; E is the
 * predicted-expression table, G x C in the problem's layout (L, or mu * L for model_mu = TRUE, :423-428).  All in float64:
 *   a_n = rowSums(Y)_n / sum_g E[g][c_n]  (:429)      r_ng = a_n E[g][c_n] - y_ng  (:430-432)
 *   sse_total = sum of r_ng^2 over the used cells and all genes; the reference's value is sse_total / (n_cells_used * G)
 *   sse_gene[g] (G values) and sse_cell[n] (N values, 0 for a skipped cell): the same sum per gene / per cell; either may be NULL.
 * The residual is formed and squared per count, sums run in a fixed order (no atomics): two calls agree bit for bit.
 * CA_ERR_INVALID (with a message): a clone index outside [-1, C), a non-finite entry of E, a clone in use whose column of E sums
 * to zero or to a non-finite value.  Sharded handle: collective; sse_total, n_cells_used and sse_gene are totals over all ranks
 * (through the engine's transport), sse_cell covers the local cells, and input refused on one rank is refused on every rank.
 * Read-only: no variable, Adam slot or draw index changes; not from a poll hook (CA_ERR_STATE), like the other sums. */
int ca_fit_mse(ca_handle h, const int32_t* clone_of_cell, const double* E, double* sse_total, int64_t* n_cells_used,
               double* sse_gene, double* sse_cell);

/* Per-cell, per-clone log-likelihood of the resident counts under a fitted model at its point estimates: the reference's p_y_on_c
 * (R/inference-tflow.R:288-296) with mu_samples replaced by the point estimate, in ONE float64 sweep over the resident counts (any
 * storage; the matrix is not shipped back and no N x G array is made).  E: expected expression, G x C, non-negative (a fit gives
 * mu_g L[g][c]); U (N x D) and V (G x D), 0 <= D <= 8: per-cell and per-gene factors of the exponent eta_ng = sum_d U[n][d] V[g][d]
 * (a fit gives U = [psi | x], V = [W | beta]); both may be NULL when D = 0.  Matrices in the problem's layout.
 *   ll[n][c] = sum_g xlogy(y_ng, E[g][c]) + sum_g y_ng eta_ng - s_n log sum_g E[g][c] exp(eta_ng) + const_n,      s_n = sum_g y_ng
 *   const_n  = lgamma(s_n + 1) - sum_g lgamma(y_ng + 1)   when with_const != 0, else 0
 * i.e. Multinomial(total = s_n, probs ~ E[.][c] exp(eta_n.)).log_prob(y_n).  Rules:
 *   xlogy: a count of 0 against E = 0 adds 0; a positive count against E = 0 makes that ll[n][c] exactly -inf; no NaN is produced,
 *     neither in that cell's other clones nor anywhere else.
 *   log sum_g E exp(eta) is taken under a per-cell shift by max_g eta_ng: it does not overflow while ll itself is representable.
 *   Everything is float64; sums run in a fixed order (no atomics): two calls agree bit for bit; a cell's row of ll does not depend on
 *     its place in the launch, so a cell-sharded group returns the single handle's bits.
 * CA_ERR_INVALID (with a message naming the clone, gene or cell): D outside [0, 8]; D > 0 with U or V NULL; an entry of E negative or
 * non-finite; a column of E that sums to zero or to a non-finite value; a non-finite entry of U or V.
 * Sharded handle: U and ll cover the local cells; the only collective is the verdict on the input, so that input refused on one
 * rank (a non-finite U is local) is refused on every rank.
 * Read-only: no variable, Adam slot or draw index changes; not from a poll hook (CA_ERR_STATE), like the other sums. */
int ca_clone_loglik(ca_handle h, const double* E /* G x C */, const double* U /* N x D, or NULL */, const double* V /* G x D, or NULL */,
                    int32_t D, int32_t with_const, double* ll /* N x C */);

/* Log-likelihood of the resident counts under a MIXTURE OF TWO CLONES -- a heterotypic doublet: the sum of two multinomial rows of clones a and b is
 * multinomial in w p_a + (1 - w) p_b -- for every unordered pair a < b, every weight of a grid and the cells [cell_lo, cell_lo + cell_cnt).  Notation and
 * arguments of ca_clone_loglik: E (G x C), eta_ng = U_n . V_g, Z_nc = sum_g E[g][c] exp(eta_ng), s_n = sum_g y_ng; U is N x D over ALL resident cells.
 *   pair_ll[n][(a,b)][w] = sum_{g: y_ng > 0} y_ng log( w E[g][a] / Z_na + (1 - w) E[g][b] / Z_nb ) + sum_g y_ng eta_ng + const_n
 * with const_n as in ca_clone_loglik.  Pairs in lexicographic order (0,1), (0,2), ..., (C-2,C-1), M = C (C - 1) / 2 of them; pair_ll is cell_cnt x (M n_weights)
 * in the problem's layout, column = pair * n_weights + weight index, row = cell - cell_lo.  ll (cell_cnt x C, or NULL): ca_clone_loglik's rows of those
 * cells, bit for bit.  Rules:
 *   the bracket is evaluated under a per-pair shift: lz = min(log Z_na, log Z_nb), coefficients w exp(lz - log Z_na) and (1 - w) exp(lz - log Z_nb), both <= 1,
 *     and s_n lz subtracted outside the sum; log Z_nc itself under the max_g eta_ng shift of ca_clone_loglik: nothing overflows while the result is representable.
 *   a positive count on a gene where BOTH clones have E = 0 makes that entry exactly -inf; E = 0 in one clone only is finite; a zero count is skipped (0 log 0 is
 *     never formed); no NaN anywhere; a cell with s_n = 0 gets 0 + const_n.
 *   With D > 0 the weight a gene sees depends on the cell (through Z_na / Z_nb): one float64 log per (cell, non-zero count, pair, weight), a wave per cell over
 *     its non-zero counts in ascending gene order, a lane per (pair, weight).  With D = 0 the logarithm is a per-gene table of M n_weights columns, swept like
 *     ca_clone_loglik's.  Everything is float64, sums run in a fixed order (no atomics): two calls agree bit for bit, and a cell's values depend neither on the
 *     cell range it was asked in nor on its place in the launch, so a cell-sharded group returns the single handle's bits.
 * CA_ERR_INVALID (with a message naming the offender): everything ca_clone_loglik refuses; C < 2; n_weights outside [1, 8]; a weight that is non-finite or
 * outside the open interval (0, 1); a cell range outside [0, N]; E or pair_ll NULL.
 * Sharded handle: U, the cell range and the outputs are the local cells'; the only collective is the verdict on the input.
 * Read-only: no variable, Adam slot or draw index changes; not from a poll hook (CA_ERR_STATE), like the other sums. */
int ca_clone_pair_loglik(ca_handle h, const double* E /* G x C */, const double* U /* N x D, or NULL */, const double* V /* G x D, or NULL */, int32_t D,
                         int32_t with_const, const double* weights /* n_weights, each in (0, 1) */, int32_t n_weights, int64_t cell_lo, int64_t cell_cnt,
                         double* ll /* cell_cnt x C, or NULL */, double* pair_ll /* cell_cnt x (M n_weights) */);

/* The maximum-likelihood MIXTURE OF ALL CLONES per cell -- a spatial spot, a bulk sample, a contaminated droplet, an off-grid doublet or a triplet: the sum of
 * multinomial rows of several clones is multinomial in sum_c pi_c p_n.c -- for the cells [cell_lo, cell_lo + cell_cnt): the weights pi on the simplex that
 * maximise it, by projected Newton, with a certified bound.  Notation and arguments of ca_clone_loglik: E (G x C; further columns may be profiles that are no
 * clone, e.g. ambient RNA), eta_ng = U_n . V_g, Z_nc = sum_g E[g][c] exp(eta_ng), s_n = sum_g y_ng; U is N x D over ALL resident cells.  Per cell, with
 * lz = min_c log Z_nc and q_gc = E[g][c] exp(lz - log Z_nc) (every factor is at most 1, so nothing overflows):
 *   mix_ll(pi) = sum_{g: y>0} y_g log m_g - s lz + sum_g y_g eta_g + const_n,    m_g = sum_c pi_c q_gc
 *   g_c   = sum_{g: y>0} y_g q_gc / m_g          (so sum_c pi_c g_c = s_eff, the counts on usable entries)
 *   H_cd  = sum_{g: y>0} y_g q_gc q_gd / m_g^2   (minus the Hessian; positive semidefinite)
 *   bound = max_c g_c - sum_c pi_c g_c           [nats; rounded up to 0 where rounding leaves it below]
 * mix_ll is concave in pi, so for any pi on the simplex max_pi' mix_ll(pi') - mix_ll(pi) <= bound (concavity and sum_c pi'_c = 1): a theorem, and the stop
 * rule.  The constraint is dropped the mixSQP way: maximise phi(pi) = f(pi) - s_eff sum_c pi_c over pi >= 0 (f(t pi) = f(pi) + s_eff log t, so the maximiser
 * has sum 1).  One round, at the current pi (sum 1):
 *   1. evaluate g, H, mix_ll and bound; stop if bound <= tol_nats or rounds == max_iter.  The returned mix_ll, grad and bound are those of the returned
 *      weights, from the same evaluation.
 *   2. gamma = g - s_eff; active set {c : pi_c <= eps and gamma_c < 0}, eps = min(1e-3, max_c |pi_c - max(pi_c + gamma_c / H_cc, 0)|) (Bertsekas).
 *   3. on the free set solve (H_FF + ridge I) d_F = gamma_F by Cholesky, ridge = 1e-12 trace(H_FF) / |F|; active components take d_c = gamma_c / H_cc.
 *   4. trial points max(pi + t d, 0) for t = 1, 1/2, 1/4, 1/8: the largest t whose phi is finite and phi(trial) >= phi(pi) + 1e-4 gamma . (trial - pi);
 *      if none passes (or the solve breaks down) the round takes one EM step pi_c g_c / s_eff, which never lowers f.
 *   5. renormalise to sum 1 (phi does not decrease under it).
 * A round keeps no state but pi -- T rounds in one call are T calls of one round, bit for bit -- and a weight that reached 0 comes back as soon as its
 * gamma_c > 0.  start: cell_cnt x C in the problem's layout, rows on the simplex, or NULL for uniform weights.  Outputs, row = cell - cell_lo: weights
 * (cell_cnt x C), grad (cell_cnt x C or NULL: g_c / s_eff, which is 1 on the support of an optimum and <= 1 + bound / s_eff elsewhere), mix_ll, bound_nats
 * and rounds (cell_cnt each); ll (cell_cnt x C, or NULL): ca_clone_loglik's rows of those cells, bit for bit.  Rules:
 *   a positive count on a gene whose every q_gc is 0 makes mix_ll exactly -inf; such entries are left out of m, g and H, and the weights and the bound are
 *     those of the remaining entries.  Zero counts are never visited.  A cell with s_n = 0 (or no usable entry) returns the start, mix_ll = const_n, bound 0,
 *     rounds 0.  No NaN anywhere.
 *   with max_iter > 0 a start at which mix_ll is -inf on an otherwise usable entry (the start's zeros exclude the data) is replaced by the uniform start.
 *   max_iter = 0 evaluates at the start, zeros included: a one-hot start reproduces ca_clone_loglik's value and (w, 1 - w) on a pair ca_clone_pair_loglik's,
 *     to rounding.  Where the start's zeros exclude a usable entry, mix_ll is -inf, bound_nats +inf, and grad leaves those entries out.
 *   Everything is float64; a wave per cell over its compacted non-zero counts, all rounds in one launch; every sum runs in a fixed order (no atomics): two calls
 *     agree bit for bit, and a cell's values depend neither on the cell range it was asked in, nor on the batching, nor on its place in the launch, so a
 *     cell-sharded group returns the single handle's bits.
 * CA_ERR_INVALID (with a message naming the offender): everything ca_clone_loglik refuses; C > 32; max_iter < 0; tol_nats negative or non-finite; a start row
 * with a negative or non-finite entry or whose sum is off 1 by more than 1e-9; a cell range outside [0, N]; E, weights, mix_ll, bound_nats or rounds NULL.
 * Sharded handle: U, the cell range, start and the outputs are the local cells'; the only collective is the verdict on the input.
 * Read-only: no variable, Adam slot or draw index changes; not from a poll hook (CA_ERR_STATE), like the other sums. */
int ca_clone_mixture(ca_handle h, const double* E /* G x C */, const double* U /* N x D, or NULL */, const double* V /* G x D, or NULL */, int32_t D, int32_t with_const,
                     const double* start /* cell_cnt x C on the simplex, or NULL: uniform */, int32_t max_iter, double tol_nats, int64_t cell_lo, int64_t cell_cnt,
                     double* ll /* cell_cnt x C, or NULL */, double* weights /* cell_cnt x C */, double* grad /* cell_cnt x C, or NULL */, double* mix_ll,
                     double* bound_nats, int32_t* rounds /* each cell_cnt */);

/* DIRICHLET-MULTINOMIAL log-likelihood of the resident counts under every clone at a grid of concentrations, for the cells [cell_lo, cell_lo + cell_cnt):
 * scoring that allows for the overdispersion of the counts relative to ca_clone_loglik's multinomial.  Notation and arguments of ca_clone_loglik: E (G x C),
 * eta_ng = U_n . V_g, Z_nc = sum_g E[g][c] exp(eta_ng), s_n = sum_g y_ng, p_ngc = E[g][c] exp(eta_ng) / Z_nc; U is N x D over ALL resident cells.  For a
 * concentration phi_k > 0, with a_ngc = phi_k p_ngc:
 *   dm_ll[n][c][k] = lgamma(phi_k) - lgamma(phi_k + s_n) + sum_{g: y_ng > 0} [ lgamma(y_ng + a_ngc) - lgamma(a_ngc) ] + const_n
 * with const_n as in ca_clone_loglik, i.e. DirichletMultinomial(total = s_n, alpha = phi_k p_n.c).log_prob(y_n).  As phi -> inf it tends to ca_clone_loglik's
 * value; for a cell with one read it is log p_ngc at every phi.  dm_ll is cell_cnt x (C n_conc) in the problem's layout, column = clone * n_conc + k,
 * row = cell - cell_lo.  ll (cell_cnt x C, or NULL): ca_clone_loglik's rows of those cells, bit for bit.  Rules:
 *   a zero count adds nothing and is never visited; a positive count against E[g][c] = 0 makes that entry exactly -inf; no NaN anywhere; a cell with s_n = 0
 *     gets 0 + const_n.  An a_ngc that UNDERFLOWS to 0 although E > 0 (an exponent far below the cell's largest, or a vanishing share of E) is treated like E = 0.
 *   log Z_nc is ca_clone_loglik's, under the max_g eta_ng shift m_n, and is not computed a second time; the coefficient phi_k exp(m_n - log Z_nc) of a
 *     (clone, concentration) is formed once per cell and is at most phi_k, exp(eta_ng - m_n) at most 1: nothing overflows.
 *   counts may be non-integer (f32 storage) and as large as the storage allows.  An integer count y <= 8 is evaluated as log prod_{j < y} (a + j) while every
 *     concentration is at most 2^100 (the product of 8 factors below 2^101 cannot overflow); every other count by two lgamma.
 *   Everything is float64, one transcendental per (cell, non-zero count, clone, concentration), a wave per cell over its non-zero counts in ascending gene
 *     order, a lane per (clone, concentration); sums run in a fixed order (no atomics): two calls agree bit for bit, and a cell's values depend neither on the
 *     cell range it was asked in, nor on the batching, nor on its place in the launch, so a cell-sharded group returns the single handle's bits.
 * CA_ERR_INVALID (with a message naming the offender): everything ca_clone_loglik refuses; n_conc outside [1, 16]; a concentration that is non-finite or <= 0
 * (or above 1e300, where lgamma of it overflows); a cell range outside [0, N]; E, conc or dm_ll NULL.
 * Sharded handle: U, the cell range and the outputs are the local cells'; the only collective is the verdict on the input.
 * Read-only: no variable, Adam slot or draw index changes; not from a poll hook (CA_ERR_STATE), like the other sums. */
int ca_clone_loglik_dm(ca_handle h, const double* E /* G x C */, const double* U /* N x D, or NULL */, const double* V /* G x D, or NULL */, int32_t D,
                       int32_t with_const, const double* conc /* n_conc, each finite and > 0 */, int32_t n_conc, int64_t cell_lo, int64_t cell_cnt,
                       double* ll /* cell_cnt x C, or NULL */, double* dm_ll /* cell_cnt x (C n_conc), column = clone * n_conc + k */);

/* The log-likelihood of ca_clone_loglik BY BLOCK OF GENES (chromosomes, arms, copy-number segments): its four sufficient statistics per cell and block, for the
 * cells [cell_lo, cell_lo + cell_cnt).  The multinomial factorises exactly over any partition of the genes, ll[n][c] = sum_b within[n][b][c] + between[n][c], and
 * the likelihood with one block left out is again a multinomial over the remaining genes; both follow from
 *   A[n][b][c]    = sum_{g in b} xlogy(y_ng, E[g][c]) + sum_{g in b} y_ng eta_ng
 *   s[n][b]       = sum_{g in b} y_ng
 *   lg[n][b]      = sum_{g in b} lgamma(y_ng + 1)
 *   logZ[n][b][c] = log sum_{g in b} E[g][c] exp(eta_ng)
 * Notation and input rules of ca_clone_loglik (eta_ng = U_n . V_g; U is N x D over ALL resident cells).  block_of_gene[g] in [0, n_blocks) is the gene's block.
 * A and logZ are cell_cnt x (n_blocks C), column = block * C + clone; s and lg are cell_cnt x n_blocks; all in the problem's layout, row = cell - cell_lo.  Rules:
 *   a positive count against E = 0 makes that A[n][b][c] exactly -inf, a zero count adds 0; no NaN anywhere.
 *   logZ is taken under a shift by the block's max of eta (nothing overflows while the result is representable) and is -inf where the sum is 0.
 *   an empty block (a label no gene carries) gives A = 0, s = 0, lg = 0, logZ = -inf.
 *   block_of_gene may be ANY labelling: interleaved labels are legal, only slower (the sweep stores its sums at every change of label, and the cells are
 *     taken in smaller batches).
 *   Everything is float64, sums run in a fixed order (ascending genes within a block; no atomics): two calls agree bit for bit, and a cell's values depend
 *     neither on the cell range it was asked in, nor on the engine's internal batching, nor on its place in the launch, so a cell-sharded group returns the
 *     single handle's bits.
 * One sweep over the resident matrix in its storage for A, s and lg; logZ never reads it (D > 0: a contraction per block; D = 0: a host table).
 * CA_ERR_INVALID (with a message naming the offender): everything ca_clone_loglik refuses; n_blocks < 1; a label outside [0, n_blocks); a cell range outside
 * [0, N]; E, block_of_gene or an output NULL (lg may be NULL only with with_const == 0, and is not written then).
 * Sharded handle: U, the cell range and the outputs are the local cells'; the only collective is the verdict on the input.
 * Read-only: no variable, Adam slot or draw index changes; not from a poll hook (CA_ERR_STATE), like the other sums. */
int ca_clone_loglik_by_block(ca_handle h, const double* E /* G x C */, const double* U /* N x D, or NULL */, const double* V /* G x D, or NULL */, int32_t D,
                             int32_t with_const, const int32_t* block_of_gene /* G, each in [0, n_blocks) */, int32_t n_blocks, int64_t cell_lo, int64_t cell_cnt,
                             double* A /* cell_cnt x (n_blocks C) */, double* logZ /* cell_cnt x (n_blocks C) */, double* s /* cell_cnt x n_blocks */,
                             double* lg /* cell_cnt x n_blocks, or NULL when with_const == 0 */);

/* BOOTSTRAP SUPPORT FOR CLONE CALLS: ca_clone_loglik's score with the genes REWEIGHTED, for R sets of weights at once, for the cells
 * [cell_lo, cell_lo + cell_cnt).  Resampling the genes with replacement gives integer weights (how often a gene was drawn); the share of replicates that repeat
 * a cell's call says how sure the call is.  Notation and input rules of ca_clone_loglik (E is G x C, eta_ng = U_n . V_g, U is N x D over ALL resident cells);
 * w is R x G, row-major whatever the problem's layout, every entry finite and >= 0, no row all zero:
 *   A_r[n][c]    = sum_g w_rg xlogy(y_ng, E[g][c])
 *   s_r[n]       = sum_g w_rg y_ng
 *   logZ_r[n][c] = log sum_g w_rg E[g][c] exp(eta_ng)
 *   ll_r[n][c]   = A_r[n][c] - s_r[n] logZ_r[n][c]
 * For integer weights this is ca_clone_loglik (with_const = 0) of the matrix with column g repeated w_rg times, MINUS sum_g w_rg y_ng eta_ng: that term and the
 * lgamma constant are the same for every clone of a cell, change no posterior and no argmax, and are left out.
 * The reduced form is the normal output (R x N x C doubles are 640 MB at 100k cells, 8 clones, R = 100).  With t_r = ll_r + log_prior (log_prior: N x C over ALL
 * resident cells in the problem's layout, NULL = 0, -inf excludes a clone; NaN and +inf are refused):
 *   votes[n][c]    (int32) the number of replicates whose argmax_c t_r is c, ties to the lowest clone
 *   prob_sum[n][c], prob_sq[n][c]   sum_r softmax_c(t_r) and sum_r softmax_c(t_r)^2, r ascending (a replicate whose t_r is -inf in every clone votes for clone 0
 *                  and adds nothing to either)
 * all cell_cnt x C in the problem's layout, row = cell - cell_lo.  ll (or NULL: not written) is cell_cnt x (R C), column = r * C + clone; reads (or NULL) is
 * cell_cnt x R, s_r.  Rules:
 *   ll_r = -inf exactly where a positive count with a positive weight meets E = 0; a zero weight or a zero count adds nothing.  No NaN anywhere: the -inf is set
 *     from a mask before anything is subtracted (never -inf - s (-inf)), and s_r[n] = 0 gives ll_r[n][:] = 0 whatever logZ_r is.
 *   the exponent's shift is ca_clone_loglik's: per cell and chunk of CA_LL_ZCHUNK genes the max of eta over EVERY gene of the chunk, the chunks merged in
 *     ascending order under their overall max; a zero weight behaves there as E = 0 does.
 *   Everything is float64 on v_mfma_f64_16x16x4_f64 (cells x (replicate, clone) over the genes), no atomics, every sum in a fixed order: two calls agree bit for
 *     bit.  The call cuts R into chunks of CA_BOOT_RCHUNK replicates and the cells into batches; no value depends on either cut, on the cell range or on R --
 *     one call with R replicates returns what R calls with one each return -- so a cell-sharded group returns the single handle's bits.
 *   any storage (u8 with its overflow list -- escaped counts enter with their true values --, u16, f32), dense or sparse uploads, both layouts.
 * CA_ERR_INVALID (with a message naming the offender): everything ca_clone_loglik refuses; R < 1; a weight that is negative or non-finite (replicate and gene
 * are named); a replicate whose weights are all zero; log_prior NaN or +inf; a cell range outside [0, N]; E, w, votes, prob_sum or prob_sq NULL.
 * Sharded handle: U, log_prior, the cell range and the outputs are the local cells'; the only collective is the verdict on the input.
 * Read-only: no variable, Adam slot or draw index changes; not from a poll hook (CA_ERR_STATE), like the other sums. */
#define CA_BOOT_RCHUNK 32   /* replicates per chunk of ca_clone_loglik_reweighted (mirrored in clonealign_amd/engine.py) */
int ca_clone_loglik_reweighted(ca_handle h, const double* E /* G x C */, const double* U /* N x D, or NULL */, const double* V /* G x D, or NULL */, int32_t D,
                               const double* w /* R x G, row-major */, int32_t R, const double* log_prior /* N x C, or NULL */, int64_t cell_lo, int64_t cell_cnt,
                               double* ll /* cell_cnt x (R C), or NULL */, int32_t* votes /* cell_cnt x C */, double* prob_sum /* cell_cnt x C */,
                               double* prob_sq /* cell_cnt x C */, double* reads /* cell_cnt x R: s_r, or NULL */);
/* the kernel time (ms, HIP events around the launches, no copy) of the calling thread's last successful ca_clone_loglik_reweighted; 0 before the first */
int ca_reweighted_kernel_ms(double* ms);

/* Project cells onto a fitted model: for every resident cell the MAP value of its latent factor psi_n under the fit's GENE-LEVEL parameters, and the
 * exact clone posterior at it -- the per-cell part of the model for cells the fit never saw (no refit; every cell is independent).  Notation of
 * ca_clone_loglik: E (G x C) = mu L, V = [W | beta] (G x D, D = K + P), U_n = [psi_n | x_n] (the first K columns free, the last P given by X),
 * s_n = sum_g y_ng.  Per cell it maximises
 *   F_n(psi) = logsumexp_c( ll_nc(psi) + log_prior_nc ) - |psi|^2 / 2
 * with ll exactly ca_clone_loglik's and the reference's Normal(0, 1) prior on psi (R/inference-tflow.R:318-319); log_prior is the N x C addend
 * log alpha_c + extra_nc (NULL = 0).  Method: generalised EM, one safeguarded Newton step per round.
 *   once, one sweep over the resident counts:  A_nc = sum_g xlogy(y, E_gc) (+ const_n),  B_nd = sum_g y_ng V_gd,  s_n
 *   round t = 0 .. max_iter - 1, for every cell not yet frozen:
 *     1. eta_g = U_n . V_g, m = max_g eta_g; per clone Z0_c = sum_g E_gc e^(eta_g - m), Z1_c[k] = sum_g E_gc e^(eta_g - m) W_gk,
 *        Z2_c[k][l] = sum_g E_gc e^(eta_g - m) W_gk W_gl (k <= l)
 *     2. ll_c = A_c + U_n . B_n - s_n (m + log Z0_c);  gamma = softmax_c(ll + log_prior); clones at -inf get 0
 *     3. mean_c = Z1_c / Z0_c, cov_c = Z2_c / Z0_c - mean_c mean_c^T;  g = B_n[:K] - s_n sum_c gamma_c mean_c - psi;
 *        H = I + s_n sum_c gamma_c cov_c (symmetric positive definite);  d = H^-1 g, scaled to max-norm max_step when max|d| exceeds it;  psi += d
 *     4. the cell is FROZEN when max|d| (before scaling) <= tol -- before the update is applied; its outputs are those of step 2 of that round
 *   cells that reach max_iter without freezing get one more evaluation of steps 1-2 (ll / clone_probs belong to the returned psi), converged = 0.
 * Outputs: psi (N x K), ll (N x C, at psi), clone_probs (N x C), objective (N: F_n), rounds (N: rounds evaluated -- t + 1 for a cell frozen in round t,
 * max_iter otherwise), converged (N).  psi_start (N x K) or NULL = 0.  A cell whose ll + log_prior is -inf in every clone keeps its starting psi and gets
 * NaN probabilities, objective -inf, rounds = 0 and converged = 0; no NaN reaches any other cell.  K = 0: ca_clone_loglik followed by the softmax, zero
 * rounds, converged = 1.  with_const: bit 0 as in ca_clone_loglik; bits 8..15: rounds between two host reads of the frozen flags, after which no further
 * round is queued once every cell is frozen (0 = every 4th round) -- a cell's result depends on its own row alone, so this changes no result.
 * Matrices in the problem's layout; everything float64, sums in a fixed order, no atomics: two calls agree bit for bit, and a cell-sharded group returns
 * the single handle's bits.
 * K <= 2 IS THE DEVICE LIMIT: the moment kernel keeps C_group x (1 + K + K (K + 1) / 2) float64 accumulators per lane -- 24 for eight clones at K = 1, 48 at
 * K = 2, 120 at K = 4, which does not fit (open: the two-pass form, per-clone first moments and then ONE gamma-weighted second moment).
 * CA_ERR_INVALID (with a message naming the offender): K outside [0, 2]; K + P outside [0, 8]; V NULL with K + P > 0; X NULL with P > 0; max_iter < 0;
 * tol or max_step non-positive or non-finite; ca_clone_loglik's refusals on E and V; a non-finite entry of X or psi_start; a +inf or NaN in log_prior
 * (-inf is allowed: the clone is excluded for that cell).
 * Sharded handle: the cell-indexed arrays cover the local cells; the only collective is the verdict on the input.
 * Read-only: no variable, Adam slot or draw index changes; not from a poll hook (CA_ERR_STATE), like the other sums. */
int ca_project_cells(ca_handle h, const double* E /* G x C */, const double* V /* G x (K + P), or NULL */, int32_t K, int32_t P,
                     const double* X /* N x P, or NULL */, const double* log_prior /* N x C, or NULL */, const double* psi_start /* N x K, or NULL = 0 */,
                     int32_t with_const, int32_t max_iter, double tol, double max_step, double* psi /* N x K */, double* ll /* N x C */,
                     double* clone_probs /* N x C */, double* objective /* N */, int32_t* rounds /* N */, uint8_t* converged /* N */);

/* The clone evidence with psi integrated out: for every resident cell n and clone c
 *   evidence_nc = log Integral Normal(psi; 0, I_K) Multinomial(y_n | p_n.c(psi)) dpsi
 * under a fit's GENE-LEVEL parameters -- the quantity that can be compared between fits (and between numbers of factors K) on cells the fits never saw;
 * ca_project_cells' value at the MAP psi is a maximum over psi and never prefers the smaller model.  Notation of ca_project_cells.  With psi in R^K
 *   f_nc(psi) = A_nc + psi . B_n[:K] + x_n . B_n[K:] - s_n log Z_c(psi, x_n) - |psi|^2 / 2,   Z_c = sum_g E_gc exp(psi . W_g + x_n . beta_g)
 * is strictly concave in psi.  Per (cell, clone):
 *   once, one sweep over the resident counts:  A, B, s as in ca_project_cells
 *   1. MODE: safeguarded Newton from psi_start_n (the same start for every clone; NULL = 0).  Round t = 0 .. max_iter - 1, for every pair not yet frozen:
 *      m = max_g eta_g, Z0, Z1[k], Z2[k][l] as in ca_project_cells but at the PAIR's psi;  mean = Z1 / Z0, cov = Z2 / Z0 - mean mean^T;
 *      g = B_n[:K] - s_n mean - psi,  H = I + s_n cov,  d = H^-1 g (closed form for K <= 2), scaled to max-norm max_step when max|d| exceeds it;  psi += d.
 *      The pair is FROZEN when max|d| (before scaling) <= tol -- before the update is applied; f* = f(psi) and H are that round's.
 *      A pair that reaches max_iter without freezing gets one more evaluation of f and H at the psi it holds and converged = 0: H is positive definite
 *      everywhere, so its values below are deterministic, but they are NOT to be trusted.
 *   2. LAPLACE: H = L L^T (Cholesky, closed form), laplace_nc = f* - sum_k log L_kk  (the (2 pi)^(K/2) factors cancel against the prior's normaliser).
 *   3. QUADRATURE: nodes z_q (n_nodes x K, row-major ALWAYS) and weights w_q of a rule for the standard normal measure (sum w_q = 1; a Gauss-Hermite tensor
 *      rule, say).  psi_q = psi* + L^-T z_q, and
 *        evidence_nc = laplace_nc + log sum_q w_q exp( f(psi_q) - f* + |z_q|^2 / 2 ),   the sum under a running maximum in ascending q.
 *      n_nodes = 1 with z = 0 and w = 1 gives the Laplace value, bit for bit.
 * Outputs: evidence, laplace (N x C), psi_mode (N x (C K), column c K + k), psi_prec (N x (C K (K + 1) / 2), column c K (K + 1) / 2 + j: the entries of H with
 * k <= l, row by row), rounds (N x C: rounds evaluated -- t + 1 for a pair frozen in round t, max_iter otherwise), converged (N x C).  Rules:
 *   a pair with A_nc = -inf (a positive count against E = 0): evidence = laplace = -inf, rounds 0, converged 0, psi_mode = the start, psi_prec = I; no NaN anywhere.
 *   s_n = 0: the mode is 0 and evidence = laplace = 0 (to the rounding of sum w_q).
 *   K = 0: evidence = laplace = ca_clone_loglik's value bit for bit, zero rounds, converged 1 (0 where the value is -inf); nodes may be NULL.
 * with_const: bit 0 as in ca_clone_loglik; bits 8..15: rounds between two host reads of the pairs' states, as in ca_project_cells -- no result depends on it.
 * Matrices in the problem's layout; everything float64, sums in a fixed order, no atomics: two calls agree bit for bit, a cell's outputs depend on its own row
 * alone, and a cell-sharded group returns the single handle's bits.  K <= 2 is the device limit, as for ca_project_cells.
 * CA_ERR_INVALID (with a message naming the offender): everything ca_project_cells refuses (K outside [0, 2]; K + P outside [0, 8]; V NULL with K + P > 0; X NULL
 * with P > 0; max_iter < 0; tol or max_step non-positive or non-finite; ca_clone_loglik's refusals on E and V; a non-finite entry of X or psi_start); n_nodes
 * outside [1, 64]; nodes (K > 0) or weights NULL; a non-finite node; a weight that is not positive and finite; weights whose sum is off 1 by more than 1e-12.
 * Sharded handle: the cell-indexed arrays cover the local cells; the only collective is the verdict on the input.
 * Read-only: no variable, Adam slot or draw index changes; not from a poll hook (CA_ERR_STATE), like the other sums. */
int ca_clone_evidence(ca_handle h, const double* E /* G x C */, const double* V /* G x (K + P), or NULL */, int32_t K, int32_t P,
                      const double* X /* N x P, or NULL */, const double* psi_start /* N x K, or NULL = 0 */, int32_t with_const,
                      int32_t n_nodes, const double* nodes /* n_nodes x K */, const double* weights /* n_nodes */,
                      int32_t max_iter, double tol, double max_step,
                      double* evidence /* N x C */, double* laplace /* N x C */,
                      double* psi_mode /* N x (C K) */, double* psi_prec /* N x (C K(K+1)/2), H entries k <= l */,
                      int32_t* rounds /* N x C */, uint8_t* converged /* N x C */);

/* The data side of plot_clonealign() (R/plotting.R:177-205: the dense t(logcounts), its N*G-row long table, the per-gene mean and
 * sd and the per (clone, gene) means of the z-scores) as sums from ONE sweep over the resident counts (any storage; nothing N x G
 * is made on the host).  group_of_cell[n] in [0, n_groups), or -1 for a cell left out of every sum and count; n_groups in [1, 64].
 * size_factor: N values, or NULL for library-size factors centred at 1 over the used cells, sf_n = rowSums(Y)_n / mean(rowSums(Y))
 * (the engine's float64 row sums; scater's normalize() default).  All in float64:
 *   lc_ng = log2(y_ng / sf_n + 1)                                     (logcounts, :177)
 *   S1[g][q] = sum over the cells of group q of lc_ng                 (G x n_groups, the problem's layout)
 *   S2[g]    = sum over all used cells of lc_ng^2                     (G values)
 *   n_group[q] = cells of group q                                     (n_groups values)
 * from which mean_g = sum_q S1[g][q] / n, var_g = (S2[g] - n mean_g^2) / (n - 1) (:188-189) and the mean z-score of a group,
 * (S1[g][q] / n_group[q] - mean_g) / sd_g (:195-200), follow on the host.  Sums run in a fixed order (no atomics): two calls agree
 * bit for bit.  CA_ERR_INVALID (with a message naming the cell or group): a group index outside [-1, n_groups), n_groups outside
 * [1, 64], a used cell whose size factor is <= 0 or not finite (a zero library size among them, as in scater).
 * Sharded handle: collective, with the same n_groups and the same NULL-ness of size_factor on every rank; S1, S2 and n_group are
 * totals over all ranks and the default size factors use the mean over all ranks' used cells (through the engine's transport);
 * input refused on one rank is refused on every rank.
 * Read-only: no variable, Adam slot or draw index changes; not from a poll hook (CA_ERR_STATE), like the other sums. */
int ca_logexpr_sums(ca_handle h, const int32_t* group_of_cell, int32_t n_groups, const double* size_factor, double* S1, double* S2,
                    int64_t* n_group);

/* Fetch (:424-434).  name in {"mu","clone_probs","s","alpha","beta","psi","W","chi"} (the
 * reference's ml_params) or a raw variable {"loc","ls","gamma_logits","alpha_unconstr","v"}.
 * Output is float64 in the problem's layout; sizes: mu/loc/ls G, clone_probs/gamma_logits
 * N*C, s N, alpha/alpha_unconstr C, beta G*P, psi N*K, W G*K, chi/v K. */
int ca_get_param(ca_handle h, const char* name, double* out);
/* Overwrite a raw variable (same names as above, raw set + "psi","W","beta"); resets nothing else. */
int ca_set_param(ca_handle h, const char* name, const double* in);
/* d ELBO / d variable as the last pass that made it left it, raw-variable names as in ca_set_param.  After ca_gradients(): all of them, at the current state
 * and that call's draw.  The loop's passes store the gradients they make in the same buffers, whether or not they step, so after ca_iterate / ca_run they hold:
 *   loc, ls, W, beta, psi      stored by a train pass's update launches only: the gradient the LAST train pass applied -- the state before its Adam step,
 *                              its draw;
 *   gamma_logits               fused loop (ca_info.fused_sweep = 1: S = 1 up to 16 clones, mc_samples = 2 up to 8; series form or sweeps): stored by every
 *                              cell epilogue.  ca_iterate ends on a monitor pass: the state AFTER the last step and that pass's draw (called with one draw
 *                              more than the 2 n it consumes, that pass carries the next call's first forward half: then the carried draw).
 *                              Plain passes (fused_sweep = 0: mc_samples >= 3, more than 16 clones, 9..16 clones with S >= 2, the fused form switched
 *                              off): the cell epilogue stores d logits in a TRAIN pass only; a monitor pass leaves them.  After ca_iterate: with the
 *                              train variables, the state BEFORE the last step and the last train pass's draw;
 *   v, alpha_unconstr          stored by the O(K + C) body of every pass, a monitor pass's tail included (neither depends on the draw): after ca_iterate
 *                              the state AFTER the last step.
 * A cell-sharded handle (world > 1) holds the same gradients at the same states and draws: loc, ls, W, beta, v, alpha_unconstr are the gradients of the WHOLE fit
 * (made from the all-reduced sums; bit-identical on every rank), psi and gamma_logits those of the rank's own cells.  Two things differ in how it gets there:
 *   - with the vector unit's way back (ca_info.bwd_mfma = 0; K = 0 among them) a sharded ca_iterate carries no half from call to call and its train passes are
 *     plain passes even where fused_sweep = 1; its monitor passes stay fused, so gamma_logits still ends at the state AFTER the last step and the last
 *     monitor pass's draw;
 *   - ca_run ends on a plain monitor pass (no next train pass to share a sweep with), which stores no d logits: after ca_run gamma_logits belongs with the
 *     train variables -- the state before the last step and the last train pass's draw (sharded or not; 9..16 clones and mc_samples = 2 end on a fused pass).
 * tests/test_gpu_series_grad.py and tests/test_gpu_loop_grad.py read them this way, the latter for every kernel family of the loop; tests/test_gpu_shard_grad.py
 * for every rank of a sharded fit and, through ca_group_rank_handle, of a device group. */
int ca_get_gradient(ca_handle h, const char* name, double* out);

/* A new restart on the same data: what run_clonealign()'s loop (R/clonealign.R:50-56) gets by calling inference_tflow() again --
 * all eight variables at their initial values (R/inference-tflow.R:240-273: W, v, beta, alpha_unconstr, ls, gamma_logits = 0,
 * psi = psi0, loc = loc0), fresh Adam state -- without uploading the count matrix or recomputing its fit constants.
 * psi0: N x K in the problem's layout (NULL when K = 0); loc0: G values or NULL for the loc ca_create() started from. */
int ca_reinit(ca_handle h, const double* psi0, const double* loc0);

/* accumulated HIP-event time per profiled kernel class since the last reset; ca_set_profile changes the mask */
int ca_get_kernel_times(ca_handle h, double ms[CA_KERNEL_COUNT], int64_t launches[CA_KERNEL_COUNT]);
int ca_reset_kernel_times(ca_handle h);
int ca_set_profile(ca_handle h, int32_t mask);

/* built-in eps stream (Philox4x32-10 + Box-Muller), host side: out[n] for draw `draw` */
int ca_eps_draw(uint64_t seed, uint64_t draw, int64_t n, float* out);

/* Allele-specific addend of the log-likelihood, needs no handle: replaces
 * construct_ai_likelihood() + beta_binomial_log_prob() (R/allele-specific.R:17-58) as evaluated at
 * R/inference-tflow.R:166-187 with alt = t(cov) - t(ref).  Host matrices in `layout` (ca_layout): clone_allele [V, C]
 * copy number of each clone at each variant, cov / ref [N, V] coverage and reference read counts per cell; out [N, C]
 * is what ca_problem.extra_loglik takes.  The term has no parameters, so it is computed once per fit.
 * err (optional, >= 256 bytes) receives the message on failure. */
int ca_allele_loglik(int64_t N, int32_t V, int32_t C, int32_t layout, const double* clone_allele, const double* cov,
                     const double* ref, int32_t device, double* out, char* err);

/* Gene / cell filters of preprocess_for_clonealign() (R/preprocess.R:93-147), needs no handle.
 * The two O(N G) statistics -- colSums(Y) and, after the gene filters, rowSums(Y[, kept]) -- are taken on the device
 * from the caller's raw matrix (any ca_dtype, either layout, host or device pointer); the O(G) decisions follow the
 * reference's order: copy number above max (:114-116), colSums <= min_counts_per_gene (:118-120), outlying gene means
 * (mean + nmads * mad, :59-63,123-128), equal copy number in all clones (:131-135), rowSums <= min_counts_per_cell
 * (:138-139).  Outputs: keep_gene [G], keep_cell [N] (1 = retained); gene_sums [G] / cell_sums [N] optional (may be NULL).
 * The caller subsets Y, L and the names with the masks (the reference returns the filtered matrices). */
typedef struct ca_preprocess_params {
  double min_counts_per_gene;         /* 20   */
  double min_counts_per_cell;         /* 100  */
  int32_t remove_outlying_genes;      /* 1    */
  int32_t remove_genes_same_copy_number; /* 1 */
  double nmads;                       /* 10   */
  double max_copy_number;             /* 6    */
} ca_preprocess_params;
int ca_preprocess(int64_t N, int32_t G, int32_t C, int32_t layout, int32_t y_dtype, int32_t y_on_device, const void* Y,
                  const double* L, const ca_preprocess_params* params, int32_t device, uint8_t* keep_gene,
                  uint8_t* keep_cell, double* gene_sums, double* cell_sums, char* err);

/* Simulate count rows from a fitted model on the device, needs no handle: the model's generative direction,
 *   y_n ~ Multinomial(total_n, p_n),   p_ng proportional to E[g][clone_n] exp(U_n . V_g),
 * with E (G x C) = mu L, V = [W | beta] (G x D) and U_n = [psi_n | x_n] (N x D) in the notation of ca_clone_loglik.  All matrices are ROW-MAJOR host
 * arrays; Y (N x G, int32, row-major, host) receives the rows.  The sampler, per cell n with c = clone[n] and global index q = cell_offset + n:
 *   1. eta_g = sum_d U[n][d] V[g][d], products and sums rounded one by one in ascending d (0 when D = 0); m = max of eta_g over the genes with E[g][c] > 0;
 *      w_g = E[g][c] exp(eta_g - m), and w_g = 0 where E[g][c] = 0.  Float64 throughout.
 *   2. cum_g = w_0 + ... + w_g, inclusive, float64.  The device sums by a parallel scan (64-lane wave scans, sixteen wave totals, a carry per 1024 genes) and
 *      keeps the running maximum of the scanned values over the genes with w > 0, so that the table is non-decreasing and a gene with w = 0 has exactly its
 *      predecessor's value.  Its values may differ from a sequential sum's in the last bits; see "which draws can differ" below.
 *   3. draw j = 0 .. total[n] - 1: Philox4x32-10 (philox_host.h, Salmon et al., SC'11) with key (seed low 32 bits, seed high 32 bits) and counter
 *        ( j >> 1,  q low 32 bits,  draw low 32 bits,  (draw bits 32..47) | ((q >> 32) << 16) );
 *      output words (0, 1) serve even j, words (2, 3) odd j, as (lo, hi):  u = ((hi << 21 | lo >> 11) + 0.5) * 2^-53, 53 bits, in (0, 1].
 *      (total <= 2^31 - 1, draw < 2^48 and q < 2^48 are enforced, so (seed, draw, q, j) -> (key, counter, word pair) is injective.)
 *   4. t = min(u cum_{G-1}, the largest double below cum_{G-1}); the gene drawn is the first g with cum_g > t, so a gene with w_g = 0 is never drawn.
 *      Y[n][g] = the number of the cell's draws that landed on g: a row sums to total[n] exactly; total[n] = 0 gives a row of zeros.
 * Counts are integer sums of independent draws, each with its own counter: the result does not depend on the launch geometry, on the internal batching of
 * cells (device buffers stay below 256 MB) or on how a caller splits the cells -- cells [0, N) in one call equal cells [0, h) and [h, N) in two calls with
 * cell_offset = h, bit for bit, which is also how a caller shards over devices (there is no ca_group_* form).  The counters are raised with integer atomics
 * (an LDS histogram per row, or the row itself for G above about 14 000); integer addition commutes, so -- unlike the float64 sums of every other entry
 * point, which run in a fixed order without atomics -- they cannot change a bit.
 * Which draws can differ from a sequential float64 restatement (api._simulate_counts_host): only those whose t lies within rounding (the restatement flags
 * 1e-12 cum_{G-1}) of a cumulative boundary, where another grouping of the sums or the last bit of exp may pick the neighbouring gene.
 * CA_ERR_INVALID (message in err, naming the argument; nothing is written to Y): a negative or non-finite entry of E; a non-finite entry of U or V;
 * clone[n] outside [0, C); total[n] < 0 or > 2^31 - 1; total[n] > 0 for a cell whose clone has E = 0 in every gene; D outside [0, 8]; D > 0 with U or V
 * NULL; N < 0, G < 1, C < 1; N G >= 2^62; cell_offset < 0 or cell_offset + N > 2^48; draw >= 2^48.
 * err (optional, >= 256 bytes) receives the message on failure. */
int ca_simulate_counts(int64_t N, int32_t G, int32_t C, int32_t D, const double* E /* G x C */, const double* V /* G x D, or NULL */,
                       const double* U /* N x D, or NULL */, const int32_t* clone /* N */, const int64_t* total /* N */, uint64_t seed, uint64_t draw,
                       int64_t cell_offset, int32_t device, int32_t* Y /* N x G */, char* err);
/* milliseconds the k_simulate launches of the calling thread's last ca_simulate_counts took (HIP events around each launch, summed; 0 after a refusal) */
int ca_simulate_kernel_ms(double* ms);

/* Predictive check on the device, needs no handle: the statistics of n_rep replicate rows of ca_simulate_counts WITHOUT the rows.  Notation, layouts and
 * the sampler are ca_simulate_counts's.  For r = 0 .. n_rep - 1 let y^(r)_n be the row ca_simulate_counts(..., seed, draw = draw0 + r, cell_offset, ...)
 * returns for cell n -- the same row bit for bit: same table, same Philox counters, same search; it is drawn and reduced inside one block and never
 * written to global memory as a matrix.  Outputs (host, row-major):
 *   ll_rep[n][r] = Multinomial(total_n, p_n).log_prob(y^(r)_n)
 *                = lgamma(total_n + 1) - sum_g lgamma(y_g + 1) + sum over g with y_g > 0 of y_g (log E[g][c_n] + eta_g - m - log Z_n),
 *     with eta_g, m and w_g as in steps 1-2 of the sampler and Z_n = cum_{G-1}, the table's own total of the w_g; log w_g is taken as log E + eta_g - m,
 *     not as log(exp(...)).  total_n = 0 gives exactly 0; a drawn gene always has w > 0, so every value is finite.                  (N x n_rep float64)
 *   T_rep[r][g][c] = sum over the call's cells with clone[n] == c of y^(r)_ng: the pseudo-bulk totals ca_clone_gene_sums gives for observed data.
 *     May be NULL.  The caller's buffer is overwritten, not added to.                                                              (n_rep x G x C int64)
 * Float64 throughout.  The float sums run in a fixed order without atomics (a thread's genes ascending, the wave by shuffles, the block's sixteen waves
 * ascending): two calls agree bit for bit, and ll_rep of a cell depends on (seed, draw0 + r, cell_offset + n) and the cell's own inputs alone -- not on N,
 * the internal batching, n_rep, or how a caller splits the cells or the replicates between calls: replicate r of a call at draw0 equals replicate 0 of a
 * call at draw0 + r, and cells [0, N) in one call equal [0, h) and [h, N) with cell_offset = h, whose T_rep then add up.  T_rep is accumulated with
 * integer atomics in int64: exact, whatever the order of arrival.  Device buffers stay below 256 MB (the replicates go in chunks and the cells in batches that fit) as long as one replicate's
 * totals do, C x G x 8 bytes <= 64 MB; there is no ca_group_* form (shard with cell_offset).
 * CA_ERR_INVALID (message in err, naming the argument; nothing is written to ll_rep or T_rep): everything ca_simulate_counts refuses (draw0 in the place
 * of draw); n_rep < 1; draw0 + n_rep > 2^48; ll_rep NULL.  err (optional, >= 256 bytes) receives the message on failure. */
int ca_predictive_stats(int64_t N, int32_t G, int32_t C, int32_t D, const double* E /* G x C */, const double* V /* G x D, or NULL */,
                        const double* U /* N x D, or NULL */, const int32_t* clone /* N */, const int64_t* total /* N */, uint64_t seed, uint64_t draw0,
                        int32_t n_rep, int64_t cell_offset, int32_t device, double* ll_rep /* N x n_rep */, int64_t* T_rep /* n_rep x G x C, or NULL */,
                        char* err);
/* milliseconds the k_predictive launches of the calling thread's last ca_predictive_stats took (HIP events around each launch, summed; 0 after a refusal) */
int ca_predictive_kernel_ms(double* ms);

/* The moments of ca_predictive_stats's replicates in closed form, needs no handle: nothing is drawn.  Notation, layouts (row-major host arrays) and refusals are
 * ca_predictive_stats's.  Given the clones and the row sums -- what the replicates condition on -- a replicate row of cell n is ONE draw of
 * Multinomial(total_n, p_n), so the per-clone total T[g][c] is a sum of independent binomials over the clone's cells and the linear part of the row's
 * log-likelihood, sum_g y_ng log p_ng (ca_clone_loglik without the lgamma constant, at the cell's clone), is a linear statistic of one multinomial.
 * Per cell n, with c = clone[n], float64 throughout: eta_g and the shift m exactly as in step 1 of the ca_simulate_counts sampler (m = max of eta_g over
 * the genes with E[g][c] > 0); w_g = E[g][c] exp(eta_g - m), 0 where E = 0; Z = sum_g w_g in a fixed order (the largest w last); p_g = w_g / Z;
 * lp_g = log p_g taken as log E[g][c] + (eta_g - m) - log Z (not log(exp(...)); 0 and unused where E = 0) -- except for a gene with p_g > 1/2, the one
 * of largest w, where that difference cancels (|lp| may be 1e-20 under rounding noise of 1e-16): there lp_g = log1p(-(sum of the other w) / Z), which
 * keeps its relative accuracy and is 0 exactly for a lone gene; h = sum_g p_g lp_g.  Outputs (host, row-major):
 *   cell_mean[n] = total_n h                              the mean of the linear part over the replicates                                    (N float64)
 *   cell_var[n]  = total_n sum_g p_g (lp_g - h)^2         its variance, in the centred form                                                  (N float64)
 *   T_mean[g][c] = sum over the call's cells with clone[n] == c of total_n p_ng                                                           (G x C float64)
 *   T_var[g][c]  = the same sum of total_n p (1 - p)
 *   T_cum3[g][c] = the same sum of total_n p (1 - p)(1 - 2p), the third cumulant; every term is formed per (cell, gene), never as a difference of sums.
 * Exactly 0: both cell values at total_n = 0; the three columns of a clone without cells (or whose cells all have total 0); every entry with E[g][c] = 0;
 * cell_var, and the cell's share of T_var and T_cum3, where the cell's clone has one positive gene (p = 1 and lp = 0 exactly).  No NaN or inf for accepted
 * input, |eta| of several hundred included.  The caller's buffers are overwritten, not added to.
 * Sums run in a fixed order without float atomics: two calls agree bit for bit.  cell_mean and cell_var of a cell depend on its own inputs alone -- not on
 * N, the internal batching or how a caller splits the cells over calls.  The gene-side sums are grouped by the call (cells sorted by clone, in strips whose
 * length depends on N, G, C and D): across a split of the cells they add up to within rounding, not bit for bit.  D = 0: p depends on the clone alone and
 * the tables follow from the clones' sums of totals, on the host; its last bits may differ from a call with a zero factor.
 * Device buffers stay below 256 MB (the cells go in batches that fit) as long as the five tables of C x G float64 do, up to 1.6 million (gene, clone)
 * pairs; there is no ca_group_* form (the cell values need none; the tables of a split add up).
 * CA_ERR_INVALID (message in err, naming the argument; nothing is written to any output): everything ca_predictive_stats refuses about E, V, U, clone,
 * total, D, N, G and C (a cell with total > 0 whose clone has E = 0 in every gene among it); any of the five outputs NULL.  err (optional, >= 256 bytes)
 * receives the message on failure. */
int ca_predictive_moments(int64_t N, int32_t G, int32_t C, int32_t D, const double* E /* G x C */, const double* V /* G x D, or NULL */,
                          const double* U /* N x D, or NULL */, const int32_t* clone /* N */, const int64_t* total /* N */, int32_t device,
                          double* cell_mean /* N */, double* cell_var /* N */,
                          double* T_mean /* G x C */, double* T_var /* G x C */, double* T_cum3 /* G x C */, char* err);
/* milliseconds the kernel launches of the calling thread's last ca_predictive_moments took (HIP events around each launch, summed; 0 after a refusal and at D = 0) */
int ca_predictive_moments_kernel_ms(double* ms);

/* Clone separability in closed form, needs no handle and reads no counts: per cell and ORDERED pair of clones (a, b), a != b, the per-read moments of the
 * log-likelihood ratio Lambda = ll_a - ll_b of a row drawn from clone a -- a linear statistic of one multinomial -- and the per-read probability of a read
 * that rules b out.  Layouts are row-major host arrays, as for ca_predictive_moments; float64 throughout.
 *   e_gc = E[g][c] / sum_g E[g][c] (genes ascending): every output but logZ is invariant to a column's scale, and the normalisation keeps Delta small.
 *   eta_ng = U_n . V_g, d ascending, and its shift m_n exactly as in ca_clone_loglik: one chain of fused multiply-adds from 0; m_n is the max of eta over
 *   EVERY gene, taken per chunk of 512 genes, the chunks merged in ascending order under their overall max (linearly, each scaled by exp(m_chunk - m_n)).
 *   Z_nc = sum_g e_gc exp(eta_ng - m_n);  p_ncg = e_gc exp(eta_ng - m_n) / Z_nc.
 *   For a != b: S = {g: e_ga > 0 and e_gb > 0}, X = {g: e_ga > 0 and e_gb = 0}, delta_g = log e_ga - log e_gb on S (log e taken once per (gene, clone)),
 *   Delta = log Z_na - log Z_nb, d_g = delta_g - Delta (= log p_nag - log p_nbg).
 * Outputs:
 *   logZ[n][c]    = m_n + log Z_nc                                                                                                  (N x C)
 *   excl[n][a][b] = sum_{g in X} p_nag       the probability that one read of a row of clone a falls where b has copy number 0        (N x C x C)
 *   m1, m2, m3 [n][a][b] = sum_{g in S} p_nag d_g^k, k = 1, 2, 3: m1 + (what excl leaves out) is KL(p_a || p_b) per read            (N x C x C each)
 *     With factors they come from ONE float64 matrix product, cells x (C + 4 C (C - 1)) columns over the genes with exp(eta - m) on the left (the sums
 *     Z, X = sum_X e exp, M_k = sum_S e delta^k exp), by the expanded forms with q = 1 - excl:  m1 = M1/Z_a - Delta q,  m2 = M2/Z_a - 2 Delta M1/Z_a +
 *     Delta^2 q,  m3 = M3/Z_a - 3 Delta M2/Z_a + 3 Delta^2 M1/Z_a - Delta^3 q; within 1e-10 sum_S p (|delta| + |Delta|)^k of the per-gene sums.
 * Exactly 0: the diagonal a = b of the four pair outputs; excl where X is empty; m1 = m2 = m3 where the columns a and b of e are equal bit for bit
 * (E[:, b] = 2 E[:, a] included).  No NaN or inf for accepted input, |eta| = 700 included, with one exception by rule: where Z_na underflows to 0 under the
 * shift (every positive gene of a lies about 745 or more below the cell's largest exponent) logZ[n][a] = -inf and every pair entry of that cell that
 * involves a -- (a, b) and (b, a) -- is 0; the mask is applied before anything is divided.
 * Sums run in a fixed order without float atomics: two calls agree bit for bit.  A cell's values depend on its own row of U alone -- not on N, the internal
 * batching (at most 65 536 cells a batch) or the chunking of the columns -- so a caller may split the cells over calls or devices; there is no ca_group_*
 * form.  Device buffers stay below 256 MB (the cells go in batches and, for many clones, the columns in chunks) as long as sixteen cells' rows do, about
 * 300 clones.  The caller's buffers are overwritten.  D = 0: the values do not depend on the cell; the host computes one row from the per-gene sums and
 * fills all N (kernel_ms 0; last bits may differ from a call with a zero factor).
 * CA_ERR_INVALID (the message starts "ca_clone_separability: " and names the argument; nothing is written to any output): C < 2, G < 1, N < 0, D outside
 * [0, 8]; D > 0 with U or V NULL; E NULL or any output NULL; N C C >= 2^60; a negative or non-finite entry of E; a column of E that sums to 0 or to a
 * non-finite value; a non-finite entry of U or V.  N = 0 is no error.  err (optional, >= 256 bytes) receives the message on failure. */
int ca_clone_separability(int64_t N, int32_t G, int32_t C, int32_t D, const double* E /* G x C */, const double* V /* G x D, or NULL */,
                          const double* U /* N x D, or NULL */, int32_t device, double* logZ /* N x C */, double* excl /* N x C x C */,
                          double* m1 /* N x C x C */, double* m2 /* N x C x C */, double* m3 /* N x C x C */, char* err);
/* milliseconds the kernel launches of the calling thread's last ca_clone_separability took (HIP events around each launch, summed; 0 after a refusal and at D = 0) */
int ca_clone_separability_kernel_ms(double* ms);

/* The expression side of a likelihood profile over the copy-number matrix, needs no handle and reads no counts.  Notation, layouts (row-major host arrays) and
 * refusals about E, V, U, clone, total are ca_predictive_moments's, and so are eta, the shift m_n, w_g = E[g][c_n] exp(eta_g - m_n) and Z_n (the same statements,
 * the same bits).  Replacing the weight E[g][c] by mu_g kappa_j for the genes g of one block b, in clone c only, with everything else held fixed, changes the
 * total multinomial log-likelihood by gain - cost, where gain = sum_{g in b} T[g][c] (log(mu_g kappa_j) - log E[g][c]) needs the observed per-clone totals T
 * alone (ca_clone_gene_sums; the caller's part) and
 *   cost[b][c][j] = sum over the call's cells with clone[n] == c and total_n > 0 of total_n log1p(a_nbj),   a_nbj = sum_{g in b} (mu_g kappa_j - E[g][c]) x_ng,
 *   x_ng = exp(eta_ng - m_n) / Z_n                                                                                                  (B x C x J float64)
 * is this call's output.  Float64 throughout.
 * Per-gene mode (block_of_gene NULL, B == G; every gene its own block): delta = mu_g kappa_j - E (the product rounded, then the difference);
 *   a = (delta / E) p_ng with p_ng = w_g / Z_n where E > 0 (p = 1 exactly where w = Z), a = delta x_ng where E = 0; a >= -1 always.
 * Block mode (block_of_gene[g] in [0, B), any labelling, B <= 2048): per (cell, block) the two shares A = sum_{g in b} mu_g x_ng and S = sum_{g in b} p_ng, each
 *   summed in an order fixed by the labelling alone; a = max(kappa_j A - S, -1).  Two rules keep what a sum of rounded shares cannot: S = 1 exactly where the
 *   block holds every gene with E[g][c] > 0 of the cell's clone and S = min(sum, 1 - 2^-53) where it does not (so a > -1 there, however the shares round), and
 *   the entry is 0 where every gene of the block has mu_g kappa_j == E[g][c] bit for bit.
 * Exactly 0: a clone without cells in the call, cells with total_n = 0 (they join no sum), an entry whose delta is 0 (an empty block included).
 * -inf, and only there: where a = -1 for a cell with reads -- per gene, mu_g kappa_j = 0 on a gene with p_ng = 1 (the clone's only expressed gene, or one
 * beside which every other weight of the cell vanishes in float64: w = Z); in block mode, kappa_j A = 0 on a block that holds every expressed gene of the
 * clone.  The caller's gain is -inf there as well whenever the counts are possible under E.  No NaN for accepted input as long as exp(eta_g - m_n) stays finite
 * for the genes with E[g][c] = 0 too (m_n is the largest eta over the genes with E > 0; about 709 above it the term overflows to +inf).
 * Sums run in a fixed order without float atomics: two calls agree bit for bit.  The sums over cells are grouped by the call (cells listed by clone, in strips
 * whose length depends on N, G, C, D, J and B alone), so across a split of the cells the tables add up to within rounding, not bit for bit.  D = 0: x depends
 * on the clone alone and the host does the whole call in O(G C J + N); its last bits may differ from a call with a zero factor.  Device buffers stay below
 * 64 MB per kind (the cells go in batches that fit) as long as C x J x B float64 do; there is no ca_group_* form (the tables of a split add up).
 * CA_ERR_INVALID (the message starts "ca_copy_number_profile: " and names the argument; nothing is written to cost): everything ca_predictive_moments refuses
 * about E, V, U, clone, total, D, N, G and C; mu, kappa or cost NULL; a negative or non-finite entry of mu or kappa; J outside [1, 16]; block_of_gene NULL with
 * B != G; a label outside [0, B); B > 2048 in block mode (use per-gene mode for a block per gene).  N = 0 is no error: zeros.  The caller's buffer is
 * overwritten.  err (optional, >= 256 bytes) receives the message on failure. */
int ca_copy_number_profile(int64_t N, int32_t G, int32_t C, int32_t D, const double* E /* G x C */, const double* V /* G x D, or NULL */,
                           const double* U /* N x D, or NULL */, const int32_t* clone /* N */, const int64_t* total /* N */,
                           const double* mu /* G, finite, >= 0 */, int32_t J, const double* kappa /* J, finite, >= 0 */,
                           int32_t B, const int32_t* block_of_gene /* G, or NULL: per-gene mode */, int32_t device, double* cost /* B x C x J */, char* err);
/* milliseconds the kernel launches of the calling thread's last ca_copy_number_profile took (HIP events around each launch, summed; 0 after a refusal and at D = 0) */
int ca_copy_number_profile_kernel_ms(double* ms);

/* ------------------------------------------------------------------------------------------------------------------------------
 * ONE fit, cell-sharded over several devices of ONE process (ABI 6; SURVEY.md section 8b "multi-GPU via one process / 8 devices,
 * communicator created per fit", section 8e).  The reference's caller is a single R session: inference_tflow() is called once
 * (R/clonealign.R:262-280) and must come back with the whole fit.  A group holds one engine handle per entry of `devices`, rank r
 * on the cells cell_range(N, r, W) = [N r / W, N (r + 1) / W) of the problem, each driven by its own host thread (rank 0 by the
 * CALLING thread, so a poll hook runs where R's API may be used), joined by the first transport that passes the known-answer test
 * (ca_comm_selftest) on every rank:
 *     one-shot peer-to-peer by address (ca_p2p_*: the ranks' slabs are mapped by their own addresses, peer access between the
 *     devices)  ->  RCCL (ncclCommInitRank from the W threads)  ->  a host reduction between the threads (always available).
 * A transport that was committed and then failed its test leaves engines that cannot take another one: the group re-creates
 * them (second upload) and moves on -- ca_group_info says what happened and why.  The fit is the single-handle fit up to the
 * grouping of the fp64 cell sums; the ranks' replicated variables are bit-identical, and every call below returns what the
 * one-handle call of the same name returns, for ALL cells (cell-indexed outputs are gathered in the problem's layout).
 *
 * problem: as for ca_create, holding ALL cells (host pointers; a device pointer only when every rank is on that device);
 * loc0 = NULL and ca_group_init_psi_pca work sharded (sums completed over the transport).  opts: as for ca_create; device, rank and
 * world are ignored.  devices: n_devices HIP ordinals, rank order; an ordinal may repeat (test rigs on one GPU: host transport, or
 * peer-to-peer with CA_VARX_P2P_SAME_DEVICE).  transport: 0 = the chain above, or ONE ca_transport to insist on (error if it fails).
 * Calls on one group are made from one thread at a time, always the same one. */
typedef struct ca_group* ca_group_handle;
typedef struct ca_group_info {
  int32_t world;
  int32_t transport;          /* ca_transport in use */
  int32_t p2p_status;         /* 0 not tried, 1 in use, -1 set-up failed (no peer access, repeated device ...), -2 known-answer test failed */
  int32_t rccl_status;        /* same */
  int32_t rebuilds;           /* times the engines were created again after a committed transport failed */
  int32_t selftest_rounds;    /* all-reduces of the known-answer test the transport in use passed */
  int64_t N;                  /* all cells */
  char note[384];             /* why transports were skipped, in words */
} ca_group_info;
int ca_group_create(const ca_problem* problem, const ca_options* opts, const int32_t* devices, int32_t n_devices, int32_t transport,
                    ca_group_handle* out);
/* ca_group_create with the count matrix in compressed form (ca_create_sparse's contract; problem->Y must be NULL): rank r takes its
 * cells as a cell_index subset over the same compressed arrays (host CSR: its rows' runs only).  Device arrays only when every rank
 * is on that device.  The arrays are read during the call only. */
int ca_group_create_sparse(const ca_problem* problem, const ca_sparse* y, const ca_options* opts, const int32_t* devices,
                           int32_t n_devices, int32_t transport, ca_group_handle* out);
int ca_group_destroy(ca_group_handle g);
const char* ca_group_last_error(ca_group_handle g);   /* g may be NULL: the last failed ca_group_create on this thread */
int ca_group_get_info(ca_group_handle g, ca_group_info* info);
int ca_group_rank_handle(ca_group_handle g, int32_t rank, ca_handle* h);   /* read-only use (ca_get_info, ca_get_gradient, ca_get_kernel_times ...), between two group calls */
/* the one-handle calls, collectively on every rank; eps arguments are shared by the ranks (every rank must see the same draws) */
int ca_group_init_psi_pca(ca_group_handle g, const double* noise /* N x K, all cells, or NULL */, int32_t n_iter, uint64_t seed, double* pcs_out);
int ca_group_gamma_init(ca_group_handle g, const float* eps);
int ca_group_elbo(ca_group_handle g, const float* eps, double* elbo);
int ca_group_step(ca_group_handle g, const float* eps);
/* poll: called on the calling thread (rank 0's); its decision is handed to the other ranks, which wait for it at the same iteration */
int ca_group_run_ex(ca_group_handle g, int32_t max_iter, double rel_tol, const float* eps_stream, int64_t n_draws, double* elbo_trace,
                    int32_t* n_elbo, ca_poll_fn poll, void* user);
int ca_group_iterate(ca_group_handle g, int32_t n_iter, const float* eps_stream, int64_t n_draws, double* last_elbo);
int ca_group_final_elbo(ca_group_handle g, int32_t n_rep, const float* eps_stream, int64_t n_draws, double* values, double* mean, double* sd);
int ca_group_get_param(ca_group_handle g, const char* name, double* out);
int ca_group_reinit(ca_group_handle g, const double* psi0 /* N x K, all cells */, const double* loc0);
int ca_group_clone_gene_sums(ca_group_handle g, const int32_t* clone_of_cell /* N, all cells */, double* T, double* Syy);
/* ca_fit_mse (R/clonealign.R:415-434) over the group: clone_of_cell and sse_cell hold ALL cells; the totals are rank 0's (every rank has the same) */
int ca_group_fit_mse(ca_group_handle g, const int32_t* clone_of_cell /* N, all cells */, const double* E, double* sse_total,
                     int64_t* n_cells_used, double* sse_gene, double* sse_cell /* N, all cells, or NULL */);
/* ca_clone_loglik (R/inference-tflow.R:288-296) over the group: U and ll hold ALL cells (sliced by the shards); each cell's row is the single handle's, bit for bit */
int ca_group_clone_loglik(ca_group_handle g, const double* E, const double* U /* N x D, all cells, or NULL */, const double* V, int32_t D,
                          int32_t with_const, double* ll /* N x C, all cells */);
/* ca_clone_pair_loglik over the group: U holds ALL cells, the cell range counts the group's cells, ll and pair_ll hold the range's rows; each cell's values are the
 * single handle's, bit for bit (every rank is called with its part of the range, an empty one included, for the verdict on the input) */
int ca_group_clone_pair_loglik(ca_group_handle g, const double* E, const double* U /* N x D, all cells, or NULL */, const double* V, int32_t D, int32_t with_const,
                               const double* weights, int32_t n_weights, int64_t cell_lo, int64_t cell_cnt, double* ll /* cell_cnt x C, or NULL */,
                               double* pair_ll /* cell_cnt x (M n_weights) */);
/* ca_clone_mixture over the group: U and start (N x C, or NULL) hold ALL cells, the cell range counts the group's cells, the outputs hold the range's rows; each
 * cell's values are the single handle's, bit for bit (every rank is called with its part of the range, an empty one included, for the verdict on the input) */
int ca_group_clone_mixture(ca_group_handle g, const double* E, const double* U /* N x D, all cells, or NULL */, const double* V, int32_t D, int32_t with_const,
                           const double* start /* N x C, all cells, or NULL: uniform */, int32_t max_iter, double tol_nats, int64_t cell_lo, int64_t cell_cnt,
                           double* ll /* cell_cnt x C, or NULL */, double* weights /* cell_cnt x C */, double* grad /* cell_cnt x C, or NULL */, double* mix_ll,
                           double* bound_nats, int32_t* rounds /* each cell_cnt */);
/* ca_clone_loglik_dm over the group: U holds ALL cells, the cell range counts the group's cells, ll and dm_ll hold the range's rows; each cell's values are the
 * single handle's, bit for bit (every rank is called with its part of the range, an empty one included, for the verdict on the input) */
int ca_group_clone_loglik_dm(ca_group_handle g, const double* E, const double* U /* N x D, all cells, or NULL */, const double* V, int32_t D, int32_t with_const,
                             const double* conc, int32_t n_conc, int64_t cell_lo, int64_t cell_cnt, double* ll /* cell_cnt x C, or NULL */,
                             double* dm_ll /* cell_cnt x (C n_conc) */);
/* ca_clone_loglik_by_block over the group: U holds ALL cells, the cell range counts the group's cells, the outputs hold the range's rows; each cell's values are the
 * single handle's, bit for bit (every rank is called with its part of the range, an empty one included, for the verdict on the input) */
int ca_group_clone_loglik_by_block(ca_group_handle g, const double* E, const double* U /* N x D, all cells, or NULL */, const double* V, int32_t D, int32_t with_const,
                                   const int32_t* block_of_gene, int32_t n_blocks, int64_t cell_lo, int64_t cell_cnt, double* A, double* logZ, double* s,
                                   double* lg /* or NULL when with_const == 0 */);
/* ca_clone_loglik_reweighted over the group: U and log_prior hold ALL cells, the cell range counts the group's cells, the outputs hold the range's rows; each
 * cell's values are the single handle's, bit for bit (every rank is called with its part of the range, an empty one included, for the verdict on the input) */
int ca_group_clone_loglik_reweighted(ca_group_handle g, const double* E, const double* U /* N x D, all cells, or NULL */, const double* V, int32_t D,
                                     const double* w /* R x G, row-major */, int32_t R, const double* log_prior /* N x C, all cells, or NULL */, int64_t cell_lo,
                                     int64_t cell_cnt, double* ll /* cell_cnt x (R C), or NULL */, int32_t* votes, double* prob_sum, double* prob_sq,
                                     double* reads /* cell_cnt x R, or NULL */);
/* ca_project_cells over the group: X, log_prior, psi_start and every output hold ALL cells (sliced by the shards); each cell's results are the single handle's, bit for bit */
int ca_group_project_cells(ca_group_handle g, const double* E, const double* V, int32_t K, int32_t P, const double* X /* N x P, all cells, or NULL */,
                           const double* log_prior /* N x C, all cells, or NULL */, const double* psi_start /* N x K, all cells, or NULL */,
                           int32_t with_const, int32_t max_iter, double tol, double max_step, double* psi, double* ll, double* clone_probs,
                           double* objective, int32_t* rounds, uint8_t* converged);
/* ca_clone_evidence over the group: X, psi_start and every output hold ALL cells (sliced by the shards); each cell's results are the single handle's, bit for bit */
int ca_group_clone_evidence(ca_group_handle g, const double* E, const double* V, int32_t K, int32_t P, const double* X /* N x P, all cells, or NULL */,
                            const double* psi_start /* N x K, all cells, or NULL */, int32_t with_const, int32_t n_nodes, const double* nodes, const double* weights,
                            int32_t max_iter, double tol, double max_step, double* evidence, double* laplace, double* psi_mode, double* psi_prec,
                            int32_t* rounds, uint8_t* converged);
/* ca_logexpr_sums (R/plotting.R:177-205) over the group: group_of_cell and size_factor (or NULL) hold ALL cells; the totals are rank 0's (every rank has the same) */
int ca_group_logexpr_sums(ca_group_handle g, const int32_t* group_of_cell /* N, all cells */, int32_t n_groups,
                          const double* size_factor /* N, all cells, or NULL */, double* S1, double* S2, int64_t* n_group);

#ifdef __cplusplus
}
#endif
#endif /* CLONEALIGN_HIP_H */
