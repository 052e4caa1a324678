// ca_eng_state.inc -- part of clonealign_hip.hip (textually included there, in this order; one translation unit): engine state (struct ca_engine), error / launch macros, profiling wrappers, variant switches, template dispatch of the VALU sweeps and of the vector count-matrix stream, host matrix helpers.
namespace {

thread_local std::string g_last_error;

// ---- RCCL, loaded lazily so that single-GPU use never touches it
typedef struct { char internal[128]; } ca_nccl_uid;
typedef void* ca_nccl_comm;
struct RcclApi {
  void* lib = nullptr;
  int (*GetUniqueId)(ca_nccl_uid*) = nullptr;
  int (*CommInitRank)(ca_nccl_comm*, int, ca_nccl_uid, int) = nullptr;
  int (*CommDestroy)(ca_nccl_comm) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, ca_nccl_comm, hipStream_t) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  std::string err;
  bool load() {
    if (lib) return true;
    const char* cands[] = {getenv("CLONEALIGN_RCCL_LIB"), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1",
                           "/opt/rocm/lib/librccl.so"};
    for (const char* c : cands) {
      if (!c || !*c) continue;
      lib = dlopen(c, RTLD_NOW | RTLD_LOCAL);
      if (lib) break;
    }
    if (!lib) { err = std::string("cannot dlopen librccl: ") + dlerror(); return false; }
    GetUniqueId = (decltype(GetUniqueId))dlsym(lib, "ncclGetUniqueId");
    CommInitRank = (decltype(CommInitRank))dlsym(lib, "ncclCommInitRank");
    CommDestroy = (decltype(CommDestroy))dlsym(lib, "ncclCommDestroy");
    AllReduce = (decltype(AllReduce))dlsym(lib, "ncclAllReduce");
    GetErrorString = (decltype(GetErrorString))dlsym(lib, "ncclGetErrorString");
    if (!GetUniqueId || !CommInitRank || !CommDestroy || !AllReduce) { err = "librccl lacks expected symbols"; return false; }
    return true;
  }
};
RcclApi g_rccl;
constexpr int kNcclFloat64 = 8;  // ncclDouble
constexpr int kNcclSum = 0;      // ncclSum

struct EvPair { hipEvent_t a, b; int kid; };

}  // namespace

struct ca_p2p {
  double* slab = nullptr; size_t slab_bytes = 0; int64_t cap = 0;
  std::vector<void*> opened;             // peers' slabs as mapped here (nullptr for ranks of this process' own slab)
  double** peers_dev = nullptr;          // device array [world]
  unsigned long long seq = 0;
  bool mapped = false;                   // ca_p2p_connect has mapped every peer's slab
  bool connected = false;                // ca_p2p_commit(1): the transport is the engine's all-reduce
  unsigned long long* err_host = nullptr;   // pinned: 0, or the sequence number of the first call whose wait for a peer ran out
  unsigned long long* err_dev = nullptr;    // the same word as the device sees it
  unsigned int* err_local = nullptr;        // device memory: non-zero once a call has given up (what the next calls check at entry)
  unsigned long long timeout_ticks = 0;     // bound of the device-side wait, s_memrealtime ticks (100 MHz)
};
struct ca_p2p_wire {   // what travels in a CA_P2P_HANDLE_BYTES handle
  hipIpcMemHandle_t mem; int64_t cap; int32_t rank, world, device, pid;
  uint64_t local_ptr;   // the slab's address in the exporting process: peers of the SAME process take it as it is (an IPC handle cannot be opened by the process that made it)
};
static_assert(sizeof(ca_p2p_wire) <= CA_P2P_HANDLE_BYTES, "handle too small");

// What ONE TF1-Adam step can add to a magnitude, whatever the gradients were: lr_t |m| / (sqrt(v) + eps) <= lr_t (1 - b1) / sqrt((1 - b2)(1 - b1^2 / b2))
// (Cauchy-Schwarz on the two moving averages: m = (1 - b1) sum b1^i g_i, v = (1 - b2) sum b2^i g_i^2), lr_t = lr sqrt(1 - b2^t) / (1 - b1^t) maximised over t:
// 0.727 at the defaults.  Gradients that grow by b2 / b1 per step behind a long constant run come arbitrarily close to it; max(lr, lr (1 - b1) /
// sqrt(1 - b2)) = 0.316 -- constant gradients, or one gradient after none -- is NOT a bound (tests/test_adam_bound_host.py).  < 0: no such bound (b1^2 >= b2).
inline double ca_adam_step_bound(double lr, double b1, double b2) {
  if (!(b1 >= 0 && b2 > 0 && b1 * b1 < b2 && b2 < 1 && lr > 0)) return -1.0;
  double sup = 0.0, p1 = 1.0, p2 = 1.0;
  for (int t = 1; t <= 200000; ++t) { p1 *= b1; p2 *= b2; sup = std::max(sup, std::sqrt(1.0 - p2) / (1.0 - p1)); }
  return lr * sup * (1.0 - b1) / std::sqrt((1.0 - b2) * (1.0 - b1 * b1 / b2));
}
#ifndef CA_GENE_COLS_MAXN
#define CA_GENE_COLS_MAXN 65536   // cells up to which the stream's column jobs leave the series form's cell launch (CA_VAR_GENE_RIDE, see create_impl)
#endif
struct ca_engine {
  // ---- problem
  int64_t N = 0;
  int G = 0, C = 0, K = 0, P = 0, S = 0, D = 0;  // D = K + P, or 0 when K == 0 (:279-285)
  int layout = 0;
  int nchunk = 0;
  ca_options opt{};
  int device = 0;
  hipStream_t stream = nullptr;
  // second stream: the Y pass of the next parameter state runs beside the monitor pass's forward sweep
  hipStream_t stream2 = nullptr; hipEvent_t ev_params = nullptr, ev_ydone = nullptr; bool y_pending = false, async_y = true;
  hipStream_t stream3 = nullptr;   // (highest priority)
  hipEvent_t ev_poly0 = nullptr, ev_poly1 = nullptr;
  bool poly_xmax_ready = false; float* poly_xpart = nullptr;   // series form: the merged update that made the current state left max |psi| per 256-cell piece (ca_merge_args::xpart)
  bool ys_defer_next = false;   // series form: the next one-copy stream launch leaves its finisher pending (it rides on the cell launch)
  std::string err;
  std::vector<void*> allocs;
  int64_t dev_bytes = 0;
  // ---- count matrix
  int ystore = 0, ybytes = 0, VEC = 0, Gp = 0, nseg = 0, TR = 0, nrb = 0, nrg = 0;   // nrg: rows of YTpart = blocks of 4 row blocks
  void* Y = nullptr;
  int64_t y_dev_bytes = 0;
  // overflow list of the u8 storage (entries > 255), CSR (by cell) and CSC (by gene) orders, host copy kept for setup
  int64_t n_ovf = 0;
  int64_t *ovf_rowptr = nullptr, *ovf_chunk_start = nullptr; int* ovf_col_chunk_ptr = nullptr; float* ovf_csum = nullptr; int n_ovf_chunk = 0;
  int *ovf_col = nullptr, *ovf_row2 = nullptr;
  float *ovf_val = nullptr, *ovf_val2 = nullptr;
  std::vector<int> h_orow, h_ocol; std::vector<float> h_oval;
  const ca_sparse* sp_in = nullptr;   // ca_create_sparse: the compressed count matrix (read during create_impl only)
  // ---- constants
  float* Lb = nullptr;       // [nchunk][G][8]
  double *A = nullptr, *cn = nullptr, *s64 = nullptr, *colsum = nullptr, *YtX = nullptr;
  float* s32 = nullptr;
  // ---- variables + Adam slots
  float *F = nullptr, *m_psi = nullptr, *v_psi = nullptr;           // F [N][D] = (psi | X)
  float *glogit = nullptr, *m_gl = nullptr, *v_gl = nullptr;        // [N][C]
  float *V = nullptr, *m_V = nullptr, *v_V = nullptr;               // V [G][D] = (W | beta)
  float *loc = nullptr, *ls = nullptr, *m_loc = nullptr, *v_loc = nullptr, *m_ls = nullptr, *v_ls = nullptr;
  float* loc_init = nullptr;   // loc as ca_create left it (loc0, or the device-side mu_guess): ca_reinit's default
  float *vchi = nullptr, *m_v = nullptr, *v_v = nullptr;            // [K]
  float *alpha_u = nullptr, *m_a = nullptr, *v_a = nullptr;         // [C]
  // round 4 (merged update, k_update_merged): the chi / alpha step writes the alternate buffers and the host swaps them in; the exponent
  // bound of the stepped state is then made by the next forward sweep itself (em_stale: nobody has made it yet)
  float *vchi_alt = nullptr, *alpha_u_alt = nullptr;
  bool upd_merge = false, em_stale = false;
  // ca_run: the update half of train pass i + 1 is queued before the host has seen ELBO i and gated on a word the host writes (ca_merge_args::gate)
  bool run_gate = false, gate_req = false, gate_armed = false;
  // round 5: the gated launch's relay block gives up after gate_ticks (a launch that stores nothing; not an error) -- gate_t0: host clock right before
  // that launch was queued; gate_open / gate_snap: the window between queuing it and answering it, in which a poll hook may call back into the API
  // (gate_close()); in_run: ca_run_ex is on this thread's stack (hooks may only call the read-only entry points)
  unsigned long long gate_ticks = 100000ull; std::chrono::steady_clock::time_point gate_t0;
  double ticks_per_us = 100.0;   // rate of s_memrealtime on this device (hipDeviceAttributeWallClockRate; 100 MHz on gfx950), the unit of every device-side time limit
  bool gate_open = false, gate_aborted = false, in_run = false; struct gate_snapshot* gate_snap = nullptr; struct fwd_snapshot* gate_fsnap = nullptr;
  bool run_fwd = false;    // ca_run: queue the forward sweep behind a gated update ahead of the host's decision (CA_VAR_RUN_FWD)
  bool fwd_gate = false;   // ca_run: the forward sweep being queued is behind a gated update and must look at that launch's answer (ca_cell_ptrs::gate)
  unsigned long long gate_seq = 0; unsigned long long* gate_local = nullptr;
  bool p2p_ride = false;   // sharded over the peer-to-peer transport: the sweep's column sums and the stream's finishing sums ride (allreduce(), train_bwd)
  double* gaux = nullptr; int64_t gaux_slot = -1;   // [2][5][G]: ca_merge_args::aux_in / aux_out, ping-pong; gaux_slot: the eps draw the current half belongs to (-1: none)
  int gaux_idx = 0;
  int* vmm_at = nullptr; int vmm_at_idx = 0; bool vmm_at_ready = false;   // [2][16] ordered-int range of V' (k_update_merged), the buffer in use alternates
  double dir_const = 0.0;
  float b1p = 0.f, b2p = 0.f;  // running beta powers, float32 like TF's beta*_power variables
  // ---- gradients (d ELBO / d var)
  float *g_loc = nullptr, *g_ls = nullptr, *g_V = nullptr, *g_v = nullptr, *g_a = nullptr, *g_psi = nullptr, *dgl = nullptr;
  // ---- per-pass buffers
  float* eps_dev = nullptr; int64_t eps_cap = 0;  // capacity in draws
  float *mu32 = nullptr, *Mb = nullptr, *Vs = nullptr, *vmm = nullptr, *vmm_part = nullptr, *etamax2 = nullptr;
  double* gene_part = nullptr; int ngblk = 0;
  float *Zpart = nullptr, *coef = nullptr; double* scratch = nullptr;
  double* cell_part = nullptr; int ncblk = 0;
  float *gpart = nullptr, *dFpart = nullptr; int gsplit = 1, gchunk = 0, csplit = 1; int64_t cchunk = 0; int RG = 4, ntile = 0;
  float *YWpart = nullptr, *YTpart = nullptr, *YW = nullptr; double* ytpsi = nullptr;
  double* red = nullptr; int64_t red_n = 0, off_g = 0, off_y = 0;
  // series-capable engines (h->poly) lay the buffer out as [cell sums 3 + C | Y^T psi Gp K | backward moments Q | max |psi| of every rank | gene sums G (S + D)]: what a
  // SHARDED series pass reduces is the prefix up to off_g, in one collective (round 6, late); a pass on the sweeps reduces everything, as before
  int64_t off_q = 0, off_x = 0;
  bool poly_shape = false, layout_series = false;
  bool mon_tail_local = false;      // sharded series: the pending monitor tail's local block sums are in red[0 .. 3 + C) already (made on the forward's reduction launch)
  bool poly_xslot_pending = false;  // ... and so is this rank's max |psi| slot: the next collective sums it
  int poly_xglob_steps = -1;   // sharded series: Adam steps since the state whose per-rank max |psi| the slots at off_x hold (-1: they hold nothing)
  double* elbo_dev = nullptr; int64_t elbo_cap = 0; double* terms_dev = nullptr;
  double* host_pinned = nullptr;  // 8 doubles
  bool ycache_valid = false, sums_global = false, sums_started = false;
  std::vector<double> mu_part;   // sharded with loc0 = NULL: this rank's per-gene sums of y_ng / rowMeans(Y)_n, completed over all cells in setup_global_sums
  // fused two-eps sweep (monitor pass of iteration i + forward half of train pass i+1, same parameters)
  bool fused_ok = false, look_valid = false; int64_t look_slot = 0; int frow = 8;
  // ca_iterate, ABI 6: the last sweep of a call may carry the forward half of the NEXT call's first train pass (draw 2n of a 2n + 1 draw stream); `carry` marks
  // that look-ahead as one a following ca_iterate may pick up, carry_eps keeps the draw it was made with (the next call's draw 0 must be this draw, bit for bit)
  bool carry = false, carry_builtin = false; std::vector<float> carry_eps;
  // the series form of the forward / backward contraction (ca_poly.hip; one exponent dimension, one MC sample, 3..8 clones): an overlay on the fused loop --
  // fused_pass makes Z by it and leaves the backward moments in the workspace (poly_fresh: they belong to the look-ahead half look_valid refers to),
  // train_bwd turns them into the per-gene sums, train_update reads d/dF from ONE slab (poly_df)
  // the host's look ahead at the exponent range (poly_guard): every pass of a series-capable engine leaves {seq, max|psi|, min W, max W} of ITS state in a
  // mapped ring; the pass with sequence number s decides from the entry s - CA_POLY_LAG exactly (waiting for it if need be: the queue is never more than
  // that deep) and the bound of an Adam step -- a deterministic decision, the same on every run, and never a truncated series
  int64_t n_series = 0, n_series_fallback = 0;
  double *poly_ring = nullptr, *poly_ring_dev = nullptr; uint64_t poly_seq = 0, poly_seq_base = 1, adam_steps = 0, poly_steps_at[16] = {};
  // the series form's forward moments as the moment role of its count-matrix stream's launch (CA_VAR_MOM_RIDE, ca_polymom.hip.h): the pick, the launch tag, and the
  // arguments of the pass being queued (run_fused sets them, the stream's launch site takes them)
  bool mom_ride = false; unsigned mom_tag = 0; const ca_pm_args* mom_args = nullptr;
  // the moment role behind the stream's blocks instead of in front of them (CA_VAR_MOM_LAST: ca_mom_last_pick, ca_eng_create.inc): the order in use, the slots the
  // stream's blocks leave free in one round of the launch (what the pick saw), and the role's shape (groups per moment block, reducer blocks)
  bool mom_last = false, mom_ovf_first = false; int mom_free_slots = 0, mom_per = CA_MOM_PER, mom_nred = CA_MOM_NRED;
  bool cell_mfma = false;   // ... with the backward moments of its register bins gathered by fp64 MFMA per wave (CA_VAR_CELL_MFMA, k_poly_cell<CP, LEAN, true>)
  bool cell_edge = false;   // ... lean and MFMA both: the head's loads in one round trip, the block end in one parking step (CA_VAR_CELL_EDGE, k_poly_cell<CP, true, true, true>)
  bool cell_lean = false;   // the series form's cell launch in its lean form (CA_VAR_CELL_LEAN, ca_poly.hip k_poly_cell<CP, true>)
  // CA_VAR_GENE_RIDE (ca_polygene.hip.h): the stream's column jobs leave the cell launch, and an unsharded pass runs reduction + per-gene pass + column jobs as one
  // launch from train_bwd.  red_pending: the cell launch of the look-ahead half poly_fresh refers to is queued, its reduction is not (it comes with the per-gene pass);
  // ycol_pending: the column sums of the current stream launch are still to be made (the row jobs are done) -- yfin_flush gives any earlier consumer the launch;
  // poly_nb_ub: the bin count can be no more than this (poly_guard's look ahead): sizes the reducers' share of the merged grid, enters no result
  // gene_cols: the column jobs go with the reduction (the rule in create_impl: up to CA_GENE_COLS_MAXN cells); else they stay behind the cell launch's blocks
  bool gene_cols = false;
  bool gene_ride = false, red_pending = false, ycol_pending = false; unsigned gene_tag = 0; int poly_nb_ub = 0;
  bool poly = false, poly_side = false, poly_y_defer = false, poly_fresh = false, poly_df = false /* the last backward half was the series form's: d/dF is ONE slab */; ca_poly_ws pws; float* poly_zero = nullptr; unsigned char* poly_mem = nullptr;
  float *Mb2 = nullptr, *mu32B = nullptr, *Zpart2 = nullptr; double* gene_partB = nullptr;
  bool y_defer = false;
  bool ride_ok = false;   // the Y stream's blocks ride on the forward sweep's launch (k_fwd_cell_mix_y) instead of a side stream
  bool ride_ys = false;   // ... as the one-copy int8 matrix-core stream (k_fwd_cell_mix_ys)
  bool fold_gsum = false, fold_now = false;   // small problems: the backward sweep's partials are summed inside k_final_gene
  // per-gene prologue of the next fused pass, computed ahead by the train pass before it (ca_pre_args): the loops announce
  // the next (monitor, train) eps slots in hint_*, train_update fills the alternate partial buffers, fused_pass swaps them in
  int64_t hint_A = -1, hint_B = -1, pre_A = -1, pre_B = -1;
  bool pre_valid = false, pre_ok = true, pair_elbo = true;
  double* ee_partB = nullptr;   // pair sweeps: the second draw's per-block cell sums (ca_cell_ptrs::ee_partB)
  double *gene_part_alt = nullptr, *gene_partB_alt = nullptr;
  bool bwd_ready = false; int64_t bwd_slot = -1;
  double* yw_part = nullptr; int n_yw = 0;   // block partials of sum_n psi_n.(YW)_n (k_yw_dot)
  // the riding int8 stream without a finisher launch between the sweeps: its two finishing sums ride on the backward sweep as extra
  // blocks (ca_yfin_args); until that sweep is issued they are pending, and any other consumer gets the launch (yfin_flush)
  bool yfin_split = false, yfin_pending = false;
  ca_small_args mon_tail;          // pending ELBO assembly of a fused monitor pass: rides on the next backward sweep
  bool tail_fuse = true;
  double* host_dev = nullptr;      // device view of host_pinned
  unsigned long long host_seq = 0, host_seq_next = 0;
  float* eps_stage = nullptr; size_t eps_stage_bytes = 0;   // pinned staging buffer of the eps stream (built-in or the caller's)
  hipEvent_t ev_stage = nullptr;                             // completes when the last copy out of eps_stage has been made
  bool fwd_cell = false; int ncblk_f = 0, fc_tl = 4;   // forward sweep + cell epilogue in one kernel (k_fwd_cell)
  int fc_nbig = 0;                                     // > 0: k_fwd_cell_mix, that many blocks of 16 * fc_tl cells, the rest 32-cell blocks
  bool fwd_mfma = false; int fsplit = 1, fkchunk = 1, nk32 = 1; unsigned short* Mq = nullptr;   // matrix-core forward sweep
  // round 5: balanced forward sweep of small problems (k_fwd_bal_ys): bal_q tiles per block, bal_r left-over tiles in bal_nchunk gene chunks each
  bool fwd_bal = false; int bal_q = 0, bal_r = 0, bal_nchunk = 0; unsigned long long* bal_xw = nullptr; unsigned bal_tag = 0;
  // matrix-core backward sweep (k_bwd_mfma): bf16 parts of coef, its own cell split
  // round 6, the shapes whose loop is made of plain passes (mc_samples > 2, 17..32 clones, 9..16 clones with mc_samples >= 2): the forward contraction of a plain
  // pass on the matrix cores, its (sample, clone chunk) slices two to a sixteen-column sweep (pfwd), and the way back in the sixteen-clone form per chunk pair
  bool pfwd = false; int pf_npair = 0, pf_fsplit = 1, pf_kchunk = 1; unsigned short* pf_Mq = nullptr; float* pf_Z = nullptr;
  int bwd_pairs = 0;
  bool bwd_mfma = false, bwd_frac = false, c16 = false, s2 = false, s2f = false;   // s2f: mc_samples = 2 with monitor + next train pass in one sweep (CA_VAR_S2_FUSE)
  unsigned short* coefq = nullptr; int64_t N16 = 0, cchunk_m = 0; int csplit_m = 1, nwt = 0;
  int bwd_tl = CA_BWD_TL;   // gene tiles of 16 per wave in the matrix-core backward sweep: 4, or 3 for small problems (more, shorter wave jobs)
  uint64_t draw = 0;  // built-in stream position
  hipEvent_t ev_ywdone = nullptr; bool yw_pending = false, on_side = false;
  // count-matrix products on the int8 matrix cores (ca_ymfma.hip.h): ONE tiled copy through the transposing LDS read (k_ys_mfma; K = 1), fixed-point parameter images
  bool y_ys = false, ys4 = false; int* esc_off = nullptr; unsigned* esc = nullptr; int64_t n_esc = 0;
  // the 2-bit / 4-bit image of the series form's own stream launch (CA_VAR_Y2, ca_ymfma.hip.h): n2 of a segment's eight gene blocks at 2 bits (0: no such image), the
  // private gene order per segment both ways, its own escape list; the 4-bit image stays resident beside it for the riding forms of handed-over passes
  int ys_n2 = 0; uint8_t* Ys2 = nullptr; unsigned short *y2_perm = nullptr, *y2_pos = nullptr; int* esc2_off = nullptr; unsigned* esc2 = nullptr; int64_t n_esc2 = 0;
  uint8_t* Ys = nullptr; uint4 *Wr = nullptr, *Pr = nullptr; int *Wsum = nullptr, *Psum = nullptr;
  int* ys_exps = nullptr;        // [3][2]: rotating slots, see ca_ys_quant_body
  unsigned* ys_amax = nullptr;   // [2]: exact maxima of a fresh state (k_ym_absmax), float bit patterns
  float* ys_amaxp = nullptr; int ys_nq = 0;   // [3][ys_ncap][2]: per-block maxima each quantiser run leaves for the next one
  int ys_ncap = 0, ys_namax[3] = {0, 0, 0};   // pairs a slot can hold / holds (a merged update leaves one pair per gene block and per psi block)
  bool ys_launched = false;      // a stream launch has filled the partial slabs at least once (ca_ystream_parts)
  bool ys_quant_ready = false;   // the images of the CURRENT parameter state were made by the quantiser riding on k_adam_cell
  int ys_slot = 0, ys_steps = -1, ys_RS = 256, ys_nrg = 0, ys_nseg = 0; int64_t ys_N64 = 0; float ys_step_bound = -1.f;
  double adam_bound = -1.0;      // ca_adam_step_bound of this fit's Adam settings (create_impl); < 0: none holds.  Both look-aheads rest on it: ys_step_bound, poly_step_bound
  // one-shot peer-to-peer all-reduce (ca_p2p_export / ca_p2p_connect)
  ca_p2p* p2p = nullptr;
  // ---- comm
  ca_nccl_comm comm = nullptr;
  ca_host_allreduce_fn host_ar = nullptr; void* host_ar_user = nullptr; double* host_ar_buf = nullptr; int64_t host_ar_cap = 0;
  // ---- profiling
  std::vector<EvPair> ev_pool; size_t ev_used = 0; bool prof_open = false;
  unsigned prof_seen[CA_KERNEL_COUNT] = {0, 0, 0, 0, 0};   // launches per class since ca_set_profile (sampling stride)
  double k_ms[CA_KERNEL_COUNT] = {0}; int64_t k_n[CA_KERNEL_COUNT] = {0};
  int n_cu = 256;
};

namespace {

#define HIPCK(h, call)                                                                       \
  do {                                                                                       \
    hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess) {                                                                  \
      (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                          \
      return CA_ERR_HIP;                                                                     \
    }                                                                                        \
  } while (0)

#define CACK(call)                \
  do {                            \
    int rc_ = (call);             \
    if (rc_ != CA_OK) return rc_; \
  } while (0)

// The peer-to-peer all-reduce gives up inside the kernel when a peer does not show (k_p2p_allreduce); the host learns it here,
// at every point where it has waited for the stream anyway.
int comm_check(ca_engine* h) {
  if (h->host_pinned && *reinterpret_cast<volatile unsigned int*>(h->host_pinned + 41) != 0u) {
    h->err = "a forward-sweep block gave up waiting for a chunk of a left-over tile (k_fwd_bal_ys); the engine's state is undefined";
    return CA_ERR_STATE;
  }
  if (h->host_pinned && *reinterpret_cast<volatile unsigned int*>(h->host_pinned + 43) != 0u) {
    h->err = "a reducer block of the series form's moment role gave up waiting for the moment blocks of its launch (k_ys_mfma_mom); the engine's state is undefined";
    return CA_ERR_STATE;
  }
  if (h->host_pinned && *reinterpret_cast<volatile unsigned int*>(h->host_pinned + 44) != 0u) {
    h->err = "a gene block of the series form's merged way back gave up waiting for the reducer blocks of its launch (k_poly_tail); the engine's state is undefined";
    return CA_ERR_STATE;
  }
  if (h->host_pinned && *reinterpret_cast<volatile unsigned int*>(h->host_pinned + 42) != 0u) {
    h->err = "the series form of the contraction (CA_VARX_SERIES) cannot cover this fit's exponent range: max|psi| (max W - min W) exceeds 4 x " +
             std::to_string(CA_PL_NB) + " bins' worth; the passes since are truncated -- start over without the series form";
    return CA_ERR_STATE;
  }
  if (h->p2p && h->p2p->err_host && *reinterpret_cast<volatile unsigned long long*>(h->p2p->err_host) != 0ull) {
    h->err = "peer-to-peer all-reduce #" + std::to_string(*reinterpret_cast<volatile unsigned long long*>(h->p2p->err_host)) +
             ": a peer's data did not arrive within the time limit (peer lost or out of step); this engine's transport is dead -- "
             "destroy the engine and start over in a fresh process";
    return CA_ERR_COMM;
  }
  return CA_OK;
}
#define SYNC(h)                                          \
  do {                                                   \
    HIPCK(h, hipStreamSynchronize((h)->stream));         \
    CACK(comm_check(h));                                 \
  } while (0)

template <typename T>
int dalloc(ca_engine* h, T** p, int64_t n) {
  if (n <= 0) n = 1;
  void* q = nullptr;
  hipError_t e = hipMalloc(&q, (size_t)n * sizeof(T));
  if (e != hipSuccess) {
    h->err = std::string("hipMalloc of ") + std::to_string(n * sizeof(T)) + " bytes: " + hipGetErrorString(e);
    return CA_ERR_NOMEM;
  }
  // Zeroed, and the zeroing DONE before anybody can touch the buffer.  The engine's streams are non-blocking streams: a hipMemcpy on the NULL stream
  // into a buffer whose hipMemsetAsync is still queued on h->stream is not ordered behind it.  Alone on the GPU the memset ran at once and the
  // order came out right by luck; with ANOTHER PROCESS keeping the GPU busy it ran late and zeroed what had just been uploaded -- the overflow
  // list of a 1-byte matrix, i.e. wrong fit constants for every cell with a count above 255 (round 4: profiles/r04_flake.txt).
  e = hipMemsetAsync(q, 0, (size_t)n * sizeof(T), h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) { h->err = hipGetErrorString(e); return CA_ERR_HIP; }
  h->allocs.push_back(q);
  h->dev_bytes += n * (int64_t)sizeof(T);
  *p = (T*)q;
  return CA_OK;
}

// The device memory of ONE CALL (ca_eng_init.inc, ca_eng_score.inc on an engine's stream; ca_gen_call of ca_eng_simulate.inc on its own; the engine's own buffers
// are dalloc's): what the call allocated, freed when it returns -- on every path, after waiting for the stream (queued copies read the call's host vectors until
// then: declare the owner AFTER them).  The first failed allocation or copy is kept in rc with its message in *err; later requests do nothing, so a block of
// requests is checked once.  oom: the code for hipErrorOutOfMemory -- CA_ERR_HIP on an engine, as these calls have always reported it.
struct ca_call_mem {
  hipStream_t stream;
  std::string* err;
  int oom;
  std::vector<void*> owned;
  int rc = CA_OK;
  ca_call_mem(hipStream_t stream_, std::string* err_, int oom_ = CA_ERR_HIP) : stream(stream_), err(err_), oom(oom_) {}
  explicit ca_call_mem(ca_engine* h) : ca_call_mem(h->stream, &h->err) {}
  ca_call_mem(const ca_call_mem&) = delete;
  ca_call_mem& operator=(const ca_call_mem&) = delete;
  ~ca_call_mem() { release(); }
  void release() {
    if (!owned.empty()) hipStreamSynchronize(stream);
    for (void* p : owned) hipFree(p);
    owned.clear();
  }
  bool note(hipError_t e, const std::string& what) {   // true while nothing has failed
    if (e != hipSuccess && rc == CA_OK) {
      *err = what + ": " + hipGetErrorString(e);
      rc = e == hipErrorOutOfMemory ? oom : CA_ERR_HIP;
    }
    return rc == CA_OK;
  }
  bool ok(hipError_t e, const char* what, size_t bytes) { return note(e, std::string(what) + " of " + std::to_string(bytes) + " bytes"); }
  template <typename T>
  T* alloc(int64_t count) {
    void* p = nullptr;
    if (rc != CA_OK || !ok(hipMalloc(&p, (size_t)count * sizeof(T)), "hipMalloc", (size_t)count * sizeof(T))) return nullptr;
    if (p) owned.push_back(p);
    return static_cast<T*>(p);
  }
  template <typename T>
  T* upload(const std::vector<T>& v) {   // (the copy is queued on the stream)
    T* p = alloc<T>((int64_t)v.size());
    if (p) ok(hipMemcpyAsync(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, stream), "hipMemcpyAsync", v.size() * sizeof(T));
    return rc == CA_OK ? p : nullptr;
  }
};

// ---- profiling wrappers ------------------------------------------------------------------
int prof_flush(ca_engine* h) {
  if (h->ev_used == 0) return CA_OK;
  SYNC(h);
  if (h->stream2) HIPCK(h, hipStreamSynchronize(h->stream2));
  if (h->stream3) HIPCK(h, hipStreamSynchronize(h->stream3));
  for (size_t i = 0; i < h->ev_used; ++i) {
    float ms = 0.f;
    HIPCK(h, hipEventElapsedTime(&ms, h->ev_pool[i].a, h->ev_pool[i].b));
    h->k_ms[h->ev_pool[i].kid] += ms;
    h->k_n[h->ev_pool[i].kid] += 1;
  }
  h->ev_used = 0;
  return CA_OK;
}
int prof_begin(ca_engine* h, int kid) {
  h->prof_open = false;
  if (!((h->opt.profile >> kid) & 1)) return CA_OK;
  // bits 8..15 of the mask: sampling stride - 1.  An event pair costs the stream 5-6 us (two markers the packet processor drains
  // the queue for): timing every 8th launch keeps the live measurement and leaves the timed region alone.
  const unsigned stride = ((unsigned)h->opt.profile >> 8 & 0xFFu) + 1u;
  if (h->prof_seen[kid]++ % stride != 0) return CA_OK;
  if (h->ev_used == h->ev_pool.size()) {
    if (h->ev_pool.size() < 2048) {
      EvPair p; p.kid = kid;
      HIPCK(h, hipEventCreate(&p.a));
      HIPCK(h, hipEventCreate(&p.b));
      h->ev_pool.push_back(p);
    } else {
      CACK(prof_flush(h));
    }
  }
  h->ev_pool[h->ev_used].kid = kid;
  HIPCK(h, hipEventRecord(h->ev_pool[h->ev_used].a, h->stream));
  h->prof_open = true;
  return CA_OK;
}
int prof_end(ca_engine* h) {
  if (!h->prof_open) return CA_OK;
  h->prof_open = false;
  HIPCK(h, hipEventRecord(h->ev_pool[h->ev_used].b, h->stream));
  h->ev_used++;
  return CA_OK;
}
#define LAUNCH(h, kid, ...)                 \
  do {                                      \
    CACK(prof_begin(h, kid));               \
    __VA_ARGS__;                            \
    HIPCK(h, hipGetLastError());            \
    CACK(prof_end(h));                      \
  } while (0)

inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
// grid of `threads`-wide blocks for `total` elements, one thread each, flattened by ca_flat_index(): x stays below 2^22 blocks (2^30 work-items)
inline dim3 ca_grid_flat(int64_t total, int threads) {
  const int64_t nb = (total + threads - 1) / threads;
  const int64_t gx = std::min<int64_t>(nb, (int64_t)1 << 22);
  return dim3((unsigned)std::max<int64_t>(gx, 1), (unsigned)std::max<int64_t>((nb + gx - 1) / std::max<int64_t>(gx, 1), 1));
}

// Configuration comes from ca_options (variant_off / variant_on / tune).  The RELEASE library reads no tuning from the process
// environment at all; a timing-lab build (-DCA_LAB, tools/lab/) consults it when CLONEALIGN_DEBUG_ENV is set (tools/tune.py,
// tools/fuzz_parity.py): NAME=0 switches a variant off, NAME=<n> sets a parameter.
#ifdef CA_LAB
inline bool debug_env() { return getenv("CLONEALIGN_DEBUG_ENV") != nullptr; }
#else
constexpr bool debug_env() { return false; }
#endif
inline bool variant_on(const ca_engine* h, unsigned bit, const char* env) {
  if (h->opt.variant_off & bit) return false;
  if (debug_env()) if (const char* e = getenv(env)) return atoi(e) != 0;
  return true;
}
inline bool variantx_on(const ca_engine* h, unsigned bit, const char* env) {   // opt-in variants (ca_options.variant_on)
  if (h->opt.variant_on & bit) return true;
  if (debug_env()) if (const char* e = getenv(env)) return atoi(e) != 0;
  return false;
}
// Opt-in variants that were measured slower than what ships (rounds 2-5; DESIGN_HISTORY.md, profiles/) and whose code has been deleted: ca_create refuses the
// bits, in every build, instead of ignoring them.
#define CA_RETIRED_VARX (CA_VARX_Y_MFMA2 | CA_VARX_RIDE_SEQ | CA_VARX_BAL_TILES)
inline int tune_val(const ca_engine* h, int id, const char* env) {
  int v = h->opt.tune[id];
  if (v == 0 && debug_env()) if (const char* e = getenv(env)) { v = atoi(e); if (id == CA_TUNE_FC_NBIG && v == 0) v = -1; }
  return v;
}
inline bool verbose(const ca_engine* h) { return (h->opt.variant_off & CA_OPT_VERBOSE) || (debug_env() && getenv("CA_VERBOSE")); }

// Split count s in [1, smax] for a grid of xb * s equal blocks on `slots` resident block slots: fewest rounds per unit
// of work (a grid just past a multiple of the slots runs a nearly empty last round), every extra split charged
// `penalty` (its partial results are written and re-read).  Ties go to the smaller split.
inline int pick_split(int64_t xb, int64_t slots, int smax, double penalty) {
  int best = 1;
  double best_score = -1e30;
  for (int s = 1; s <= smax; ++s) {
    const int64_t B = xb * s;
    const int64_t rounds = (B + slots - 1) / slots;
    const double score = (double)B / (double)(rounds * slots) - penalty * s;
    if (score > best_score + 1e-9) { best_score = score; best = s; }
  }
  return best;
}

// ---- template dispatch of the sweeps -------------------------------------------------------
constexpr int kFwdR = 2;  // cells per lane of the forward sweep (R = 4 measured 5 % slower with 16 columns)
template <int NC>
void fwd_nc(int D, dim3 grid, hipStream_t st, const float* F, const float* em, const float* Vs, const float* M, float* Zp,
            int64_t N, int G, int gchunk) {
  const size_t lds = (size_t)gchunk * (CA_CW + (D > 0 ? D : 0)) * sizeof(float);
  switch (D) {
    case 0: hipLaunchKernelGGL((k_fwd_lds<NC, 0, kFwdR>), grid, dim3(CA_TB), lds, st, F, em, Vs, M, Zp, N, G, gchunk, D); break;
    case 1: hipLaunchKernelGGL((k_fwd_lds<NC, 1, kFwdR>), grid, dim3(CA_TB), lds, st, F, em, Vs, M, Zp, N, G, gchunk, D); break;
    case 2: hipLaunchKernelGGL((k_fwd_lds<NC, 2, kFwdR>), grid, dim3(CA_TB), lds, st, F, em, Vs, M, Zp, N, G, gchunk, D); break;
    default: hipLaunchKernelGGL((k_fwd_lds<NC, -1, kFwdR>), grid, dim3(CA_TB), lds, st, F, em, Vs, M, Zp, N, G, gchunk, D); break;
  }
}
void launch_fwd(int nc, int D, dim3 grid, hipStream_t st, const float* F, const float* em, const float* Vs, const float* M,
                float* Zp, int64_t N, int G, int gchunk) {
  switch (nc) {
    case 1: fwd_nc<1>(D, grid, st, F, em, Vs, M, Zp, N, G, gchunk); break;
    case 2: fwd_nc<2>(D, grid, st, F, em, Vs, M, Zp, N, G, gchunk); break;
    case 3: fwd_nc<3>(D, grid, st, F, em, Vs, M, Zp, N, G, gchunk); break;
    case 4: fwd_nc<4>(D, grid, st, F, em, Vs, M, Zp, N, G, gchunk); break;
    case 5: fwd_nc<5>(D, grid, st, F, em, Vs, M, Zp, N, G, gchunk); break;
    case 6: fwd_nc<6>(D, grid, st, F, em, Vs, M, Zp, N, G, gchunk); break;
    case 7: fwd_nc<7>(D, grid, st, F, em, Vs, M, Zp, N, G, gchunk); break;
    default: fwd_nc<8>(D, grid, st, F, em, Vs, M, Zp, N, G, gchunk); break;
  }
}

template <int NC>
void fwd16_nc(int D, dim3 grid, hipStream_t st, const float* F, const float* em, const float* Vs, const float* M, float* Zp,
              int64_t N, int G, int gchunk) {
  const size_t lds = (size_t)gchunk * (16 + (D > 0 ? D : 0)) * sizeof(float);
  switch (D) {
    case 0: hipLaunchKernelGGL((k_fwd_lds<NC, 0, kFwdR, 16>), grid, dim3(CA_TB), lds, st, F, em, Vs, M, Zp, N, G, gchunk, D); break;
    case 1: hipLaunchKernelGGL((k_fwd_lds<NC, 1, kFwdR, 16>), grid, dim3(CA_TB), lds, st, F, em, Vs, M, Zp, N, G, gchunk, D); break;
    case 2: hipLaunchKernelGGL((k_fwd_lds<NC, 2, kFwdR, 16>), grid, dim3(CA_TB), lds, st, F, em, Vs, M, Zp, N, G, gchunk, D); break;
    default: hipLaunchKernelGGL((k_fwd_lds<NC, -1, kFwdR, 16>), grid, dim3(CA_TB), lds, st, F, em, Vs, M, Zp, N, G, gchunk, D); break;
  }
}
// forward sweep over 2*C columns [A | B] of a fused two-eps pass; row stride 8 when 2C <= 8, else 16
void launch_fwd_fused(int C, int D, dim3 grid, hipStream_t st, const float* F, const float* em, const float* Vs, const float* M,
                      float* Zp, int64_t N, int G, int gchunk) {
  switch (2 * C) {
    case 10: fwd16_nc<10>(D, grid, st, F, em, Vs, M, Zp, N, G, gchunk); break;
    case 12: fwd16_nc<12>(D, grid, st, F, em, Vs, M, Zp, N, G, gchunk); break;
    case 14: fwd16_nc<14>(D, grid, st, F, em, Vs, M, Zp, N, G, gchunk); break;
    case 16: fwd16_nc<16>(D, grid, st, F, em, Vs, M, Zp, N, G, gchunk); break;
    default: launch_fwd(2 * C, D, grid, st, F, em, Vs, M, Zp, N, G, gchunk); break;   // 2, 4, 6, 8 columns
  }
}

struct BwdArgs {
  const float *coef, *F, *em, *Lb, *mu, *Vs, *V;
  float *gpart, *dFpart;
  int64_t N; int G; int64_t cchunk; int D, S, sidx, first_s, first;
};
template <int NC, int RG>
void bwd_nc(dim3 grid, hipStream_t st, const BwdArgs& a) {
#define CA_BWD(DT)                                                                                                   \
  hipLaunchKernelGGL((k_bwd<NC, DT, RG>), grid, dim3(CA_TB), 0, st, a.coef, a.F, a.em, a.Lb, a.mu, a.Vs, a.V, a.gpart, \
                     a.dFpart, a.N, a.G, a.cchunk, a.D, a.S, a.sidx, a.first_s, a.first)
  switch (a.D) {
    case 0: CA_BWD(0); break;
    case 1: CA_BWD(1); break;
    case 2: CA_BWD(2); break;
    default: CA_BWD(-1); break;
  }
#undef CA_BWD
}
template <int RG>
void bwd_rg(int nc, dim3 grid, hipStream_t st, const BwdArgs& a) {
  switch (nc) {
    case 1: bwd_nc<1, RG>(grid, st, a); break;
    case 2: bwd_nc<2, RG>(grid, st, a); break;
    case 3: bwd_nc<3, RG>(grid, st, a); break;
    case 4: bwd_nc<4, RG>(grid, st, a); break;
    case 5: bwd_nc<5, RG>(grid, st, a); break;
    case 6: bwd_nc<6, RG>(grid, st, a); break;
    case 7: bwd_nc<7, RG>(grid, st, a); break;
    default: bwd_nc<8, RG>(grid, st, a); break;
  }
}
void launch_bwd(int RG, int nc, dim3 grid, hipStream_t st, const BwdArgs& a) {
  if (RG == 1) bwd_rg<1>(nc, grid, st, a);
  else if (RG == 8) bwd_rg<8>(nc, grid, st, a);
  else bwd_rg<4>(nc, grid, st, a);
}

// ---- the vector count-matrix stream (k_ypass<YT, KK, TF>) ---------------------------------
// kk (1 .. 4) columns from `koff` on of the row products Y'.V -> YWp and of the column products Y'^T.F -> YTp, Y' = the stored counts under value transform TF
// (0 in the fit; the PCA initialisation's, ca_k_stream.hip.h); the overflow list's per-entry work as extra blocks behind the stream's `grid`
struct ca_ypass_ops { const float* F; int Dstride; const float* V; float *YWp, *YTp; int K; };
template <typename YT, int TF>
void ypass_t(ca_engine* h, const ca_ypass_ops& p, int koff, int kk, dim3 grid, const ca_ovf_args& ovf) {
  const int nb_main = grid.x;
  grid.x += ovf.nb_rows + ovf.nb_chunks;
  auto go = [&](auto kc) {
    hipLaunchKernelGGL((k_ypass<YT, decltype(kc)::value, TF>), grid, dim3(CA_TB), 0, h->stream, (const YT*)h->Y, p.F, p.Dstride, p.V, koff, p.YWp, p.YTp, h->N, h->G,
                       h->Gp, h->nseg, h->nrb, h->TR, p.K, ovf, nb_main);
  };
  switch (kk) {
    case 1: go(std::integral_constant<int, 1>()); break;
    case 2: go(std::integral_constant<int, 2>()); break;
    case 3: go(std::integral_constant<int, 3>()); break;
    default: go(std::integral_constant<int, 4>()); break;
  }
}
template <int TF>
void ypass(ca_engine* h, const ca_ypass_ops& p, int koff, int kk, dim3 grid, const ca_ovf_args& ovf) {
  if (h->ystore == CA_YSTORE_U8) ypass_t<uint8_t, TF>(h, p, koff, kk, grid, ovf);
  else if (h->ystore == CA_YSTORE_U16) ypass_t<uint16_t, TF>(h, p, koff, kk, grid, ovf);
  else ypass_t<float, TF>(h, p, koff, kk, grid, ovf);
}

// ---- host matrix helpers ------------------------------------------------------------------
// element (r, c) of an R x Cn host matrix in the problem's layout
inline int64_t hidx(int layout, int64_t r, int64_t c, int64_t R, int64_t Cn) {
  return layout == CA_COL_MAJOR ? c * R + r : r * Cn + c;
}

int upload_f(ca_engine* h, float* dst, const std::vector<float>& v) {
  if (v.empty()) return CA_OK;
  HIPCK(h, hipMemcpyAsync(dst, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
  SYNC(h);
  return CA_OK;
}
int upload_d(ca_engine* h, double* dst, const std::vector<double>& v) {
  if (v.empty()) return CA_OK;
  HIPCK(h, hipMemcpyAsync(dst, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  SYNC(h);
  return CA_OK;
}
int download_f(ca_engine* h, std::vector<float>& v, const float* src, int64_t n) {
  v.resize((size_t)n);
  if (n == 0) return CA_OK;
  HIPCK(h, hipMemcpyAsync(v.data(), src, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  SYNC(h);
  return CA_OK;
}
int read_doubles(ca_engine* h, const double* dev, double* out, int n) {
  HIPCK(h, hipMemcpyAsync(h->host_pinned, dev, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  SYNC(h);
  for (int i = 0; i < n; ++i) out[i] = h->host_pinned[i];
  return CA_OK;
}

