// ca_eng_predictive.inc -- part of clonealign_hip.hip (textually included there, after ca_eng_simulate.inc; one translation unit; ca_gen_call, the call's scaffold, is defined there): C ABI without a handle: the log-likelihoods and per-clone gene totals of replicate rows that are drawn and reduced on the device and never stored (ca_predictive_stats; include/clonealign_hip.h states the outputs), the kernel time of the calling thread's last call.
namespace { thread_local double pred_kernel_ms = 0.0; }

int ca_predictive_kernel_ms(double* ms) { return gen_kernel_ms(ms, pred_kernel_ms); }

// How a call is cut under a budget of `budget` bytes per device buffer (64 MB; four kinds of buffer, a quarter of a gigabyte in all, as for ca_simulate_counts): R replicates per chunk (the totals T [R][C][G] int64 and a cell's R values of ll
// both fit; at least one), then NB cells per batch (U, clone, total and ll [NB][R] fit; at least one).  What does not give way: ONE replicate's totals,
// C x G x 8 bytes, which pass the budget above 8.4 million (gene, clone) pairs.
extern "C++" {
namespace {
struct ca_pred_cut { int64_t R, NB; };
inline ca_pred_cut pred_cut(int64_t N, int32_t G, int32_t C, int32_t D, int32_t n_rep, bool totals, int64_t budget) {
  int64_t R = std::min<int64_t>(n_rep, std::max<int64_t>(1, budget / 8));
  if (totals) R = std::min<int64_t>(R, std::max<int64_t>(1, budget / ((int64_t)C * G * 8)));
  const int64_t NB = std::min<int64_t>(N, std::max<int64_t>(1, budget / ((int64_t)D * 8 + 12 + 8 * R)));
  return ca_pred_cut{R, NB};
}
}  // namespace
}  // extern "C++"

// Validates everything on the host before the first byte of an output is written (ca_simulate_counts's checks, then its own three).  Device buffers, each
// within the budget (pred_cut): the totals T [replicates][C][G] int64 -- clone-major, so that a wave's atomics fall on consecutive addresses; the replicates
// are taken in chunks that fit, and the host turns a chunk into the caller's [r][g][c] --, the per-block scratch (log w, and the table's and the counters'
// rows where they do not fit in LDS; the number of blocks gives way first), and a batch of cells with its ll [cells][chunk].  A value of ll depends on
// (seed, draw0 + r, cell_offset + n) and the cell's own arguments alone and T is an integer sum, so neither the chunks, the batches nor the number of
// blocks change a bit.
int ca_predictive_stats(int64_t N, int32_t G, int32_t C, int32_t D, const double* E, const double* V, const double* U, const int32_t* clone, const int64_t* total,
                        uint64_t seed, uint64_t draw0, int32_t n_rep, int64_t cell_offset, int32_t device, double* ll_rep, int64_t* T_rep, char* err) {
  ca_gen_call call("ca_predictive_stats", err, pred_kernel_ms);
  std::string bad = sim_check_shape(N, G, C, D, E, V, U, clone, total, !ll_rep, "E, clone, total and ll_rep must not be NULL", cell_offset);
  if (!bad.empty()) return call.refuse(bad);
  if (n_rep < 1) return call.refuse("n_rep = " + std::to_string(n_rep) + " is below 1");
  if (draw0 > ((uint64_t)1 << 48) || (uint64_t)n_rep > ((uint64_t)1 << 48) - draw0)
    return call.refuse("draw0 = " + std::to_string(draw0) + " with n_rep = " + std::to_string(n_rep) + ": draw0 + n_rep must not exceed 2^48");
  std::vector<double> Et, Vt;
  bad = sim_check_values(N, G, C, D, E, V, U, clone, total, Et, Vt);
  if (!bad.empty()) return call.refuse(bad);
  if (N == 0) {
    if (T_rep) std::fill(T_rep, T_rep + (size_t)n_rep * G * C, (int64_t)0);
    return CA_OK;
  }

  const ca_sim_plan plan = sim_plan(G);
  const int64_t budget = (int64_t)64 << 20;
  const ca_pred_cut cut = pred_cut(N, G, C, D, n_rep, T_rep != nullptr, budget);
  const int64_t R = cut.R, NB = cut.NB;   // replicates per chunk, cells per batch
  const int64_t per_block = (int64_t)G * (8 + (plan.S > 1 ? 8 : 0) + (plan.hist_lds ? 0 : 4));
  std::vector<double> lgt(CA_LL_LGTAB);
  for (int k = 0; k < CA_LL_LGTAB; ++k) lgt[(size_t)k] = std::lgamma((double)k + 1.0);
  int n_cu = 0;
  if (!call.open(device) || !call.note(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device), "hipDeviceGetAttribute")) return call.failed();
  const int blocks = (int)std::min<int64_t>(std::min<int64_t>(NB, 2 * (int64_t)std::max(n_cu, 1)), std::max<int64_t>(1, budget / per_block));   // two blocks per CU at the LDS plan
  call.model(Et, Vt, D, NB);
  ca_pred_ops o;
  o.Et = call.Et; o.Vt = call.Vt; o.U = call.U; o.clone = call.clone; o.total = call.total; o.G = G; o.C = C; o.D = D; o.plan = plan; o.seed = seed;
  o.lgtab = call.upload(lgt);
  o.ll = call.alloc<double>(NB * R);
  o.lw_blk = call.alloc<double>((int64_t)blocks * G);
  o.cum_blk = plan.S > 1 ? call.alloc<double>((int64_t)blocks * G) : nullptr;
  o.row_blk = plan.hist_lds ? nullptr : call.alloc<int32_t>((int64_t)blocks * G);
  o.T = T_rep ? call.alloc<unsigned long long>(R * C * G) : nullptr;
  if (o.row_blk) call.note(hipMemsetAsync(o.row_blk, 0, (size_t)blocks * G * sizeof(int32_t), call.stream), "hipMemsetAsync of the counters");
  if (call.rc != CA_OK) return call.failed();
  for (int64_t r_lo = 0; r_lo < n_rep; r_lo += R) {
    const int64_t r_cnt = std::min<int64_t>(R, n_rep - r_lo);
    if (o.T && !call.note(hipMemsetAsync(o.T, 0, (size_t)r_cnt * C * G * sizeof(unsigned long long), call.stream), "hipMemsetAsync of the totals")) return call.failed();
    o.n_rep = (int)r_cnt; o.draw0 = draw0 + (uint64_t)r_lo;
    for (int64_t n_lo = 0; n_lo < N; n_lo += NB) {
      const int64_t n_cnt = std::min<int64_t>(NB, N - n_lo);
      o.n_cnt = n_cnt; o.blocks = (int)std::min<int64_t>(blocks, n_cnt); o.q0 = (uint64_t)(cell_offset + n_lo);
      if (!call.feed(U, clone, total, n_lo, n_cnt) || !call.timed([&]() { return launch_predictive(call.stream, o); }) ||
          !call.note(hipMemcpy2D(ll_rep + (size_t)n_lo * n_rep + r_lo, (size_t)n_rep * sizeof(double), o.ll, (size_t)r_cnt * sizeof(double), (size_t)r_cnt * sizeof(double),
                                 (size_t)n_cnt, hipMemcpyDeviceToHost), "hipMemcpy2D of ll"))
        return call.failed();
    }
    // [r][c][g] on the device -> the caller's [r][g][c]
    if (o.T && !call.gene_major(o.T, r_cnt, C, G, [&](int64_t r) { return T_rep + (size_t)(r_lo + r) * G * C; })) return call.failed();
  }
  return call.done();
}
