// ca_eng_simulate.inc -- part of clonealign_hip.hip (textually included there, in this order; one translation unit): C ABI without a handle: count rows drawn from a fitted model (ca_simulate_counts; include/clonealign_hip.h has the sampler), the kernel time of the calling thread's last call.
namespace { thread_local double sim_kernel_ms = 0.0; }

int ca_simulate_kernel_ms(double* ms) {
  if (!ms) return CA_ERR_INVALID;
  *ms = sim_kernel_ms;
  return CA_OK;
}

// The refusals ca_simulate_counts and ca_predictive_stats share, in ca_simulate_counts's order; each returns the refusal's text (without the entry point's
// name), empty when there is none.  sim_check_shape: the sizes and the pointers (out_null: an output the entry point needs is NULL; null_msg says which).
// sim_check_values: every entry; fills Et [C][G] and Vt [D][G].
extern "C++" {
namespace {
std::string sim_check_shape(int64_t N, int32_t G, int32_t C, int32_t D, const double* E, const double* V, const double* U, const int32_t* clone, const int64_t* total,
                            bool out_null, const char* null_msg, int64_t cell_offset) {
  if (N < 0 || G < 1 || C < 1) return std::string("N = " + std::to_string(N) + ", G = " + std::to_string(G) + ", C = " + std::to_string(C) + ": N must be >= 0, G and C >= 1");
  if (D < 0 || D > CA_LL_DMAX) return std::string("D = " + std::to_string(D) + " is outside [0, " + std::to_string(CA_LL_DMAX) + "]");
  if (D > 0 && (!U || !V)) return std::string("D = " + std::to_string(D) + " needs both U (cells x D) and V (genes x D)");
  if ((double)N * (double)G >= 4611686018427387904.0) return std::string("N x G = " + std::to_string(N) + " x " + std::to_string(G) + " is 2^62 or more");
  if (!E || (N > 0 && (!clone || !total || out_null))) return std::string(null_msg);
  if (cell_offset < 0 || cell_offset > ((int64_t)1 << 48) - N) return std::string("cell_offset = " + std::to_string(cell_offset) + ": cell_offset + N must lie in [0, 2^48]");
  return std::string();
}
std::string sim_check_values(int64_t N, int32_t G, int32_t C, int32_t D, const double* E, const double* V, const double* U, const int32_t* clone, const int64_t* total,
                             std::vector<double>& Et, std::vector<double>& Vt) {
  Et.assign((size_t)C * G, 0.0); Vt.assign((size_t)D * G, 0.0);
  // E: transposed to [C][G] (a block reads one clone's column, gene by gene); which clones can be drawn from at all
  std::vector<char> possible((size_t)C, 0);
  for (int g = 0; g < G; ++g)
    for (int c = 0; c < C; ++c) {
      const double v = E[(size_t)g * C + c];
      if (!std::isfinite(v) || v < 0.0) return std::string("E has a negative or non-finite entry (gene " + std::to_string(g) + ", clone " + std::to_string(c) + ")");
      Et[(size_t)c * G + g] = v;
      if (v > 0.0) possible[(size_t)c] = 1;
    }
  for (int g = 0; g < G; ++g)
    for (int d = 0; d < D; ++d) {
      const double v = V[(size_t)g * D + d];
      if (!std::isfinite(v)) return std::string("V has a non-finite entry (gene " + std::to_string(g) + ", factor " + std::to_string(d) + ")");
      Vt[(size_t)d * G + g] = v;
    }
  for (int64_t n = 0; n < N; ++n) {
    for (int d = 0; d < D; ++d)
      if (!std::isfinite(U[(size_t)n * D + d])) return std::string("U has a non-finite entry (cell " + std::to_string(n) + ", factor " + std::to_string(d) + ")");
    if (clone[n] < 0 || clone[n] >= C) return std::string("clone[" + std::to_string(n) + "] = " + std::to_string(clone[n]) + " is outside [0, " + std::to_string(C) + ")");
    if (total[n] < 0 || total[n] > 2147483647) return std::string("total[" + std::to_string(n) + "] = " + std::to_string(total[n]) + " is outside [0, 2^31 - 1]");
    if (total[n] > 0 && !possible[(size_t)clone[n]])
      return std::string("total[" + std::to_string(n) + "] = " + std::to_string(total[n]) + " but E is zero in every gene of the cell's clone " + std::to_string(clone[n]));
  }
  return std::string();
}
}  // namespace
}  // extern "C++"

// Validates everything on the host before the first byte of Y is written, then runs the cells in batches whose device buffers (the int32 rows, and the
// float64 table slab when the search table has two levels) stay below a quarter of a gigabyte; a batch is one memset, one or more launches over its work
// items and a copy of its rows through two pinned chunks (the DMA of one chunk runs while the host copies the other into Y).  A cell's row depends on
// (seed, draw, cell_offset + n) and its own arguments alone, so neither the batch size nor the item list changes a bit.
int ca_simulate_counts(int64_t N, int32_t G, int32_t C, int32_t D, const double* E, const double* V, const double* U, const int32_t* clone, const int64_t* total,
                       uint64_t seed, uint64_t draw, int64_t cell_offset, int32_t device, int32_t* Y, char* err) {
  auto fail = [&](int code, const std::string& m) { if (err) { strncpy(err, m.c_str(), 255); err[255] = 0; } return code; };
  auto refuse = [&](const std::string& m) { return fail(CA_ERR_INVALID, "ca_simulate_counts: " + m); };
  sim_kernel_ms = 0.0;
  std::string bad = sim_check_shape(N, G, C, D, E, V, U, clone, total, !Y, "E, clone, total and Y must not be NULL", cell_offset);
  if (!bad.empty()) return refuse(bad);
  if (draw >> 48) return refuse("draw = " + std::to_string(draw) + " is 2^48 or more");
  std::vector<double> Et, Vt;
  bad = sim_check_values(N, G, C, D, E, V, U, clone, total, Et, Vt);
  if (!bad.empty()) return refuse(bad);
  if (N == 0) return CA_OK;

  const ca_sim_plan plan = sim_plan(G);
  const int64_t per_cell = (int64_t)G * (4 + (plan.S > 1 ? 8 : 0));
  const int64_t NB = std::min<int64_t>(N, std::max<int64_t>(1, ((int64_t)1 << 28) / per_cell));
  const size_t chunk_bytes = (size_t)std::min<int64_t>((int64_t)16 << 20, NB * (int64_t)G * 4);   // (a chunk is a run of bytes, not of rows)
  const int64_t max_items = (int64_t)1 << 20;   // work items per launch
  double *Et_d = nullptr, *Vt_d = nullptr, *U_d = nullptr, *cum_d = nullptr; int32_t *cl_d = nullptr, *Y_d = nullptr; int64_t* tot_d = nullptr; ca_sim_item* it_d = nullptr;
  char* stage[2] = {nullptr, nullptr};
  hipStream_t stream = nullptr; hipEvent_t ev[2] = {nullptr, nullptr}, done[2] = {nullptr, nullptr};
  auto cleanup = [&]() { hipFree(Et_d); hipFree(Vt_d); hipFree(U_d); hipFree(cum_d); hipFree(cl_d); hipFree(Y_d); hipFree(tot_d); hipFree(it_d);
                         for (int i = 0; i < 2; ++i) { if (stage[i]) hipHostFree(stage[i]); if (ev[i]) hipEventDestroy(ev[i]); if (done[i]) hipEventDestroy(done[i]); }
                         if (stream) hipStreamDestroy(stream); };
#define SCK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { cleanup(); return fail(e_ == hipErrorOutOfMemory ? CA_ERR_NOMEM : CA_ERR_HIP, std::string("ca_simulate_counts: " #call ": ") + hipGetErrorString(e_)); } } while (0)
  SCK(hipSetDevice(device));
  SCK(hipStreamCreate(&stream));
  for (int i = 0; i < 2; ++i) { SCK(hipEventCreate(&ev[i])); SCK(hipEventCreateWithFlags(&done[i], hipEventDisableTiming)); SCK(hipHostMalloc((void**)&stage[i], chunk_bytes)); }
  SCK(hipMalloc((void**)&Et_d, Et.size() * sizeof(double)));
  SCK(hipMemcpyAsync(Et_d, Et.data(), Et.size() * sizeof(double), hipMemcpyHostToDevice, stream));
  if (D > 0) {
    SCK(hipMalloc((void**)&Vt_d, Vt.size() * sizeof(double)));
    SCK(hipMemcpyAsync(Vt_d, Vt.data(), Vt.size() * sizeof(double), hipMemcpyHostToDevice, stream));
    SCK(hipMalloc((void**)&U_d, (size_t)NB * D * sizeof(double)));
  }
  SCK(hipMalloc((void**)&cl_d, (size_t)NB * sizeof(int32_t)));
  SCK(hipMalloc((void**)&tot_d, (size_t)NB * sizeof(int64_t)));
  SCK(hipMalloc((void**)&Y_d, (size_t)NB * G * sizeof(int32_t)));
  if (plan.S > 1) SCK(hipMalloc((void**)&cum_d, (size_t)NB * G * sizeof(double)));
  SCK(hipMalloc((void**)&it_d, (size_t)std::min<int64_t>(max_items, NB * (int64_t)((2147483647 / CA_SIM_SEG) + 1)) * sizeof(ca_sim_item)));
  std::vector<ca_sim_item> items;
  double kernel_ms = 0.0;
  for (int64_t n_lo = 0; n_lo < N; n_lo += NB) {
    const int64_t n_cnt = std::min<int64_t>(NB, N - n_lo);
    if (D > 0) SCK(hipMemcpyAsync(U_d, U + (size_t)n_lo * D, (size_t)n_cnt * D * sizeof(double), hipMemcpyHostToDevice, stream));
    SCK(hipMemcpyAsync(cl_d, clone + n_lo, (size_t)n_cnt * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    SCK(hipMemcpyAsync(tot_d, total + n_lo, (size_t)n_cnt * sizeof(int64_t), hipMemcpyHostToDevice, stream));
    SCK(hipMemsetAsync(Y_d, 0, (size_t)n_cnt * G * sizeof(int32_t), stream));
    ca_sim_ops o;
    o.Et = Et_d; o.Vt = Vt_d; o.U = U_d; o.clone = cl_d; o.total = tot_d; o.items = it_d; o.cumg = cum_d; o.Y = Y_d; o.G = G; o.D = D; o.plan = plan;
    o.seed = seed; o.draw = draw; o.q0 = (uint64_t)(cell_offset + n_lo);
    auto flush = [&]() -> hipError_t {   // one launch over the items gathered so far; the list is free to be refilled when this returns
      if (items.empty()) return hipSuccess;
      hipError_t e_ = hipMemcpyAsync(it_d, items.data(), items.size() * sizeof(ca_sim_item), hipMemcpyHostToDevice, stream);
      if (e_ == hipSuccess) e_ = hipStreamSynchronize(stream);   // (the copy has read the pageable list)
      if (e_ == hipSuccess) e_ = hipEventRecord(ev[0], stream);
      o.n_items = (int64_t)items.size();
      if (e_ == hipSuccess) e_ = launch_simulate(stream, o);
      if (e_ == hipSuccess) e_ = hipEventRecord(ev[1], stream);
      if (e_ == hipSuccess) e_ = hipEventSynchronize(ev[1]);
      float ms = 0.f;
      if (e_ == hipSuccess) e_ = hipEventElapsedTime(&ms, ev[0], ev[1]);
      kernel_ms += ms;
      items.clear();
      return e_;
    };
    for (int64_t li = 0; li < n_cnt; ++li)
      for (int64_t j = 0; j < total[n_lo + li]; j += CA_SIM_SEG) {
        items.push_back(ca_sim_item{(int32_t)li, (uint32_t)j});
        if ((int64_t)items.size() == max_items) SCK(flush());
      }
    SCK(flush());
    // the batch's rows to the caller, chunk by chunk through the two pinned buffers
    const size_t bytes = (size_t)n_cnt * G * sizeof(int32_t);
    char* dst = reinterpret_cast<char*>(Y + (size_t)n_lo * G);
    const char* src = reinterpret_cast<const char*>(Y_d);
    const size_t nchunk = (bytes + chunk_bytes - 1) / chunk_bytes;
    for (size_t k = 0; k <= nchunk; ++k) {
      if (k < nchunk) {
        const size_t off = k * chunk_bytes, len = std::min(chunk_bytes, bytes - off);
        SCK(hipMemcpyAsync(stage[k & 1], src + off, len, hipMemcpyDeviceToHost, stream));
        SCK(hipEventRecord(done[k & 1], stream));
      }
      if (k > 0) {
        const size_t off = (k - 1) * chunk_bytes, len = std::min(chunk_bytes, bytes - off);
        SCK(hipEventSynchronize(done[(k - 1) & 1]));
        memcpy(dst + off, stage[(k - 1) & 1], len);
      }
    }
  }
  SCK(hipStreamSynchronize(stream));
#undef SCK
  cleanup();
  sim_kernel_ms = kernel_ms;
  return CA_OK;
}
