// ca_eng_predictive.inc -- part of clonealign_hip.hip (textually included there, after ca_eng_simulate.inc; one translation unit): C ABI without a handle: the log-likelihoods and per-clone gene totals of replicate rows that are drawn and reduced on the device and never stored (ca_predictive_stats; include/clonealign_hip.h states the outputs), the kernel time of the calling thread's last call.
namespace { thread_local double pred_kernel_ms = 0.0; }

int ca_predictive_kernel_ms(double* ms) {
  if (!ms) return CA_ERR_INVALID;
  *ms = pred_kernel_ms;
  return CA_OK;
}

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
  auto fail = [&](int code, const std::string& m) { if (err) { strncpy(err, m.c_str(), 255); err[255] = 0; } return code; };
  auto refuse = [&](const std::string& m) { return fail(CA_ERR_INVALID, "ca_predictive_stats: " + m); };
  pred_kernel_ms = 0.0;
  std::string bad = sim_check_shape(N, G, C, D, E, V, U, clone, total, !ll_rep, "E, clone, total and ll_rep must not be NULL", cell_offset);
  if (!bad.empty()) return refuse(bad);
  if (n_rep < 1) return refuse("n_rep = " + std::to_string(n_rep) + " is below 1");
  if (draw0 > ((uint64_t)1 << 48) || (uint64_t)n_rep > ((uint64_t)1 << 48) - draw0)
    return refuse("draw0 = " + std::to_string(draw0) + " with n_rep = " + std::to_string(n_rep) + ": draw0 + n_rep must not exceed 2^48");
  std::vector<double> Et, Vt;
  bad = sim_check_values(N, G, C, D, E, V, U, clone, total, Et, Vt);
  if (!bad.empty()) return refuse(bad);
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
  double *Et_d = nullptr, *Vt_d = nullptr, *U_d = nullptr, *cum_d = nullptr, *lw_d = nullptr, *lgt_d = nullptr, *ll_d = nullptr;
  int32_t *cl_d = nullptr, *row_d = nullptr; int64_t* tot_d = nullptr; unsigned long long* T_d = nullptr;
  hipStream_t stream = nullptr; hipEvent_t ev[2] = {nullptr, nullptr};
  auto cleanup = [&]() { hipFree(Et_d); hipFree(Vt_d); hipFree(U_d); hipFree(cum_d); hipFree(lw_d); hipFree(lgt_d); hipFree(ll_d); hipFree(cl_d); hipFree(row_d); hipFree(tot_d);
                         hipFree(T_d); for (int i = 0; i < 2; ++i) if (ev[i]) hipEventDestroy(ev[i]);
                         if (stream) hipStreamDestroy(stream); };
#define PCK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { cleanup(); return fail(e_ == hipErrorOutOfMemory ? CA_ERR_NOMEM : CA_ERR_HIP, std::string("ca_predictive_stats: " #call ": ") + hipGetErrorString(e_)); } } while (0)
  PCK(hipSetDevice(device));
  int n_cu = 0;
  PCK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
  const int blocks = (int)std::min<int64_t>(std::min<int64_t>(NB, 2 * (int64_t)std::max(n_cu, 1)), std::max<int64_t>(1, budget / per_block));   // two blocks per CU at the LDS plan
  PCK(hipStreamCreate(&stream));
  for (int i = 0; i < 2; ++i) PCK(hipEventCreate(&ev[i]));
  PCK(hipMalloc((void**)&Et_d, Et.size() * sizeof(double)));
  PCK(hipMemcpyAsync(Et_d, Et.data(), Et.size() * sizeof(double), hipMemcpyHostToDevice, stream));
  PCK(hipMalloc((void**)&lgt_d, lgt.size() * sizeof(double)));
  PCK(hipMemcpyAsync(lgt_d, lgt.data(), lgt.size() * sizeof(double), hipMemcpyHostToDevice, stream));
  if (D > 0) {
    PCK(hipMalloc((void**)&Vt_d, Vt.size() * sizeof(double)));
    PCK(hipMemcpyAsync(Vt_d, Vt.data(), Vt.size() * sizeof(double), hipMemcpyHostToDevice, stream));
    PCK(hipMalloc((void**)&U_d, (size_t)NB * D * sizeof(double)));
  }
  PCK(hipMalloc((void**)&cl_d, (size_t)NB * sizeof(int32_t)));
  PCK(hipMalloc((void**)&tot_d, (size_t)NB * sizeof(int64_t)));
  PCK(hipMalloc((void**)&ll_d, (size_t)NB * R * sizeof(double)));
  PCK(hipMalloc((void**)&lw_d, (size_t)blocks * G * sizeof(double)));
  if (plan.S > 1) PCK(hipMalloc((void**)&cum_d, (size_t)blocks * G * sizeof(double)));
  if (!plan.hist_lds) {
    PCK(hipMalloc((void**)&row_d, (size_t)blocks * G * sizeof(int32_t)));
    PCK(hipMemsetAsync(row_d, 0, (size_t)blocks * G * sizeof(int32_t), stream));
  }
  std::vector<unsigned long long> T_h;
  if (T_rep) {
    PCK(hipMalloc((void**)&T_d, (size_t)R * C * G * sizeof(unsigned long long)));
    T_h.resize((size_t)R * C * G);
  }
  double kernel_ms = 0.0;
  for (int64_t r_lo = 0; r_lo < n_rep; r_lo += R) {
    const int64_t r_cnt = std::min<int64_t>(R, n_rep - r_lo);
    if (T_d) PCK(hipMemsetAsync(T_d, 0, (size_t)r_cnt * C * G * sizeof(unsigned long long), stream));
    for (int64_t n_lo = 0; n_lo < N; n_lo += NB) {
      const int64_t n_cnt = std::min<int64_t>(NB, N - n_lo);
      if (D > 0) PCK(hipMemcpyAsync(U_d, U + (size_t)n_lo * D, (size_t)n_cnt * D * sizeof(double), hipMemcpyHostToDevice, stream));
      PCK(hipMemcpyAsync(cl_d, clone + n_lo, (size_t)n_cnt * sizeof(int32_t), hipMemcpyHostToDevice, stream));
      PCK(hipMemcpyAsync(tot_d, total + n_lo, (size_t)n_cnt * sizeof(int64_t), hipMemcpyHostToDevice, stream));
      PCK(hipStreamSynchronize(stream));   // (the copies have read the caller's pageable arrays)
      ca_pred_ops o;
      o.Et = Et_d; o.Vt = Vt_d; o.U = U_d; o.clone = cl_d; o.total = tot_d; o.lgtab = lgt_d; o.cum_blk = cum_d; o.lw_blk = lw_d; o.row_blk = row_d; o.ll = ll_d; o.T = T_d;
      o.n_cnt = n_cnt; o.blocks = (int)std::min<int64_t>(blocks, n_cnt); o.G = G; o.C = C; o.D = D; o.n_rep = (int)r_cnt; o.plan = plan;
      o.seed = seed; o.draw0 = draw0 + (uint64_t)r_lo; o.q0 = (uint64_t)(cell_offset + n_lo);
      PCK(hipEventRecord(ev[0], stream));
      PCK(launch_predictive(stream, o));
      PCK(hipEventRecord(ev[1], stream));
      PCK(hipEventSynchronize(ev[1]));
      float ms = 0.f;
      PCK(hipEventElapsedTime(&ms, ev[0], ev[1]));
      kernel_ms += ms;
      PCK(hipMemcpy2D(ll_rep + (size_t)n_lo * n_rep + r_lo, (size_t)n_rep * sizeof(double), ll_d, (size_t)r_cnt * sizeof(double), (size_t)r_cnt * sizeof(double), (size_t)n_cnt,
                      hipMemcpyDeviceToHost));
    }
    if (T_d) {   // [r][c][g] on the device -> the caller's [r][g][c]
      PCK(hipMemcpy(T_h.data(), T_d, (size_t)r_cnt * C * G * sizeof(unsigned long long), hipMemcpyDeviceToHost));
      for (int64_t r = 0; r < r_cnt; ++r)
        for (int c = 0; c < C; ++c) {
          const unsigned long long* src = T_h.data() + ((size_t)r * C + c) * G;
          int64_t* dst = T_rep + (size_t)(r_lo + r) * G * C + c;
          for (int g = 0; g < G; ++g) dst[(size_t)g * C] = (int64_t)src[g];
        }
    }
  }
#undef PCK
  cleanup();
  pred_kernel_ms = kernel_ms;
  return CA_OK;
}
