// ca_eng_simulate.inc -- part of clonealign_hip.hip (textually included there, in this order; one translation unit): C ABI without a handle: the refusals and the call scaffold (ca_gen_call) of the generative family -- ca_simulate_counts here, ca_predictive_stats and ca_predictive_moments in the two files after this one --, then count rows drawn from a fitted model (ca_simulate_counts; include/clonealign_hip.h has the sampler) and the kernel time of the calling thread's last call.

// The refusals the three entry points share, in ca_simulate_counts's order; each returns the refusal's text (without the entry point's
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

// ONE HANDLE-FREE CALL of the generative family: the device, a stream and the timing event pair; the call's device memory (ca_call_mem on that stream), pinned
// staging and further events, all released when the call returns, on every path; the first HIP failure with its code (hipErrorOutOfMemory is CA_ERR_NOMEM,
// anything else CA_ERR_HIP) -- every member does nothing once something has failed, so a block of requests is checked once; the model's tables and a batch of
// cells on the device; the kernel time of the call, which reaches the thread's slot (what ca_*_kernel_ms reports) only when the call succeeds.
struct ca_gen_call : ca_call_mem {
  std::string name, msg;
  char* err_out;
  double& ms_slot;
  double kernel_ms = 0.0;
  hipEvent_t ev[2] = {nullptr, nullptr};
  std::vector<hipEvent_t> events;
  std::vector<void*> pinned;
  std::vector<char> host;   // gene_major's staging, kept between chunks
  int D = 0;
  double *Et = nullptr, *Vt = nullptr, *U = nullptr; int32_t* clone = nullptr; int64_t* total = nullptr;   // on the device: [C][G], [D][G]; a batch's [NB][D], [NB], [NB]
  ca_gen_call(const char* name_, char* err_, double& ms_slot_) : ca_call_mem(nullptr, &msg, CA_ERR_NOMEM), name(name_), err_out(err_), ms_slot(ms_slot_) { ms_slot = 0.0; }
  ~ca_gen_call() {
    if (stream) hipStreamSynchronize(stream);
    std::reverse(owned.begin(), owned.end());   // last in, first out: freed in the order of allocation, ca_predictive_moments's fifteen buffers left the allocator in a
    release();                                  // state that made every other call's hipMalloc's slow (8 .. 21 ms a call against a steady 10.5; profiles/r21_generative_refactor.txt)
    for (void* p : pinned) hipHostFree(p);
    for (hipEvent_t e : events) hipEventDestroy(e);
    for (hipEvent_t e : ev) if (e) hipEventDestroy(e);
    if (stream) hipStreamDestroy(stream);
  }
  int fail(int code, const std::string& m) { if (err_out) { strncpy(err_out, (name + ": " + m).c_str(), 255); err_out[255] = 0; } return code; }
  int refuse(const std::string& m) { return fail(CA_ERR_INVALID, m); }
  int failed() {   // the recorded failure; the stream has drained, so nothing queued still reads the caller's or the entry point's host memory
    if (stream) hipStreamSynchronize(stream);
    return fail(rc, msg);
  }
  int done() {
    if (!note(hipStreamSynchronize(stream), "hipStreamSynchronize")) return failed();
    ms_slot = kernel_ms;
    return CA_OK;
  }
  bool open(int32_t device) {
    return note(hipSetDevice(device), "hipSetDevice") && note(hipStreamCreate(&stream), "hipStreamCreate") && note(hipEventCreate(&ev[0]), "hipEventCreate") &&
           note(hipEventCreate(&ev[1]), "hipEventCreate");
  }
  hipEvent_t event() {   // (for ordering, not for timing)
    hipEvent_t e = nullptr;
    if (rc == CA_OK && note(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreateWithFlags")) events.push_back(e);
    return e;
  }
  char* staging(size_t bytes) {
    void* p = nullptr;
    if (rc == CA_OK && ok(hipHostMalloc(&p, bytes), "hipHostMalloc", bytes)) pinned.push_back(p);
    return static_cast<char*>(p);
  }
  template <typename F>
  bool timed(F&& launch) {   // one launch between the two events; its time joins the call's
    float ms = 0.f;
    if (rc == CA_OK && note(hipEventRecord(ev[0], stream), "hipEventRecord") && note(launch(), "kernel launch") && note(hipEventRecord(ev[1], stream), "hipEventRecord") &&
        note(hipEventSynchronize(ev[1]), "hipEventSynchronize") && note(hipEventElapsedTime(&ms, ev[0], ev[1]), "hipEventElapsedTime"))
      kernel_ms += ms;
    return rc == CA_OK;
  }
  void model(const std::vector<double>& Et_h, const std::vector<double>& Vt_h, int D_, int64_t NB) {   // the tables (queued) and room for a batch of NB cells
    D = D_;
    Et = upload(Et_h);
    if (D > 0) { Vt = upload(Vt_h); U = alloc<double>(NB * D); }
    clone = alloc<int32_t>(NB);
    total = alloc<int64_t>(NB);
  }
  bool feed(const double* U_h, const int32_t* clone_h, const int64_t* total_h, int64_t n_lo, int64_t n_cnt) {   // cells [n_lo, n_lo + n_cnt) are on the device when it returns
    return rc == CA_OK && (D == 0 || note(hipMemcpyAsync(U, U_h + (size_t)n_lo * D, (size_t)n_cnt * D * sizeof(double), hipMemcpyHostToDevice, stream), "hipMemcpyAsync of U")) &&
           note(hipMemcpyAsync(clone, clone_h + n_lo, (size_t)n_cnt * sizeof(int32_t), hipMemcpyHostToDevice, stream), "hipMemcpyAsync of clone") &&
           note(hipMemcpyAsync(total, total_h + n_lo, (size_t)n_cnt * sizeof(int64_t), hipMemcpyHostToDevice, stream), "hipMemcpyAsync of total") &&
           note(hipStreamSynchronize(stream), "hipStreamSynchronize");   // (the copies have read the caller's pageable arrays)
  }
  template <typename S, typename Dst>
  bool gene_major(const S* dev, int64_t K, int C, int G, Dst&& dst) {   // K tables [C][G] on the device -> dst(k)[g][c], k = 0 .. K - 1
    const size_t bytes = (size_t)K * C * G * sizeof(S);
    if (host.size() < bytes) host.resize(bytes);
    if (rc != CA_OK || !ok(hipMemcpy(host.data(), dev, bytes, hipMemcpyDeviceToHost), "hipMemcpy", bytes)) return false;
    const S* src = reinterpret_cast<const S*>(host.data());
    for (int64_t k = 0; k < K; ++k)
      for (int c = 0; c < C; ++c, src += G) {
        auto* out = dst(k) + c;
        for (int g = 0; g < G; ++g) out[(size_t)g * C] = static_cast<std::remove_reference_t<decltype(*out)>>(src[g]);
      }
    return true;
  }
};
inline int gen_kernel_ms(double* ms, double v) {
  if (!ms) return CA_ERR_INVALID;
  *ms = v;
  return CA_OK;
}
thread_local double sim_kernel_ms = 0.0;
}  // namespace
}  // extern "C++"

int ca_simulate_kernel_ms(double* ms) { return gen_kernel_ms(ms, sim_kernel_ms); }

// Validates everything on the host before the first byte of Y is written, then runs the cells in batches whose device buffers (the int32 rows, and the
// float64 table slab when the search table has two levels) stay below a quarter of a gigabyte; a batch is one memset, one or more launches over its work
// items and a copy of its rows through two pinned chunks (the DMA of one chunk runs while the host copies the other into Y).  A cell's row depends on
// (seed, draw, cell_offset + n) and its own arguments alone, so neither the batch size nor the item list changes a bit.
int ca_simulate_counts(int64_t N, int32_t G, int32_t C, int32_t D, const double* E, const double* V, const double* U, const int32_t* clone, const int64_t* total,
                       uint64_t seed, uint64_t draw, int64_t cell_offset, int32_t device, int32_t* Y, char* err) {
  ca_gen_call call("ca_simulate_counts", err, sim_kernel_ms);
  std::string bad = sim_check_shape(N, G, C, D, E, V, U, clone, total, !Y, "E, clone, total and Y must not be NULL", cell_offset);
  if (!bad.empty()) return call.refuse(bad);
  if (draw >> 48) return call.refuse("draw = " + std::to_string(draw) + " is 2^48 or more");
  std::vector<double> Et, Vt;
  bad = sim_check_values(N, G, C, D, E, V, U, clone, total, Et, Vt);
  if (!bad.empty()) return call.refuse(bad);
  if (N == 0) return CA_OK;

  const ca_sim_plan plan = sim_plan(G);
  const int64_t per_cell = (int64_t)G * (4 + (plan.S > 1 ? 8 : 0));
  const int64_t NB = std::min<int64_t>(N, std::max<int64_t>(1, ((int64_t)1 << 28) / per_cell));
  const size_t chunk_bytes = (size_t)std::min<int64_t>((int64_t)16 << 20, NB * (int64_t)G * 4);   // (a chunk is a run of bytes, not of rows)
  const int64_t max_items = (int64_t)1 << 20;   // work items per launch
  call.open(device);
  hipEvent_t arrived[2]; char* stage[2];
  for (int i = 0; i < 2; ++i) { arrived[i] = call.event(); stage[i] = call.staging(chunk_bytes); }
  call.model(Et, Vt, D, NB);
  ca_sim_ops o;
  o.Et = call.Et; o.Vt = call.Vt; o.U = call.U; o.clone = call.clone; o.total = call.total; o.G = G; o.D = D; o.plan = plan; o.seed = seed; o.draw = draw;
  o.Y = call.alloc<int32_t>(NB * G);
  o.cumg = plan.S > 1 ? call.alloc<double>(NB * G) : nullptr;
  ca_sim_item* it_d = call.alloc<ca_sim_item>(std::min<int64_t>(max_items, NB * (int64_t)((2147483647 / CA_SIM_SEG) + 1)));
  o.items = it_d;
  if (call.rc != CA_OK) return call.failed();
  std::vector<ca_sim_item> items;
  auto flush = [&]() {   // one launch over the items gathered so far; the list is free to be refilled when this returns
    if (!items.empty() && call.note(hipMemcpyAsync(it_d, items.data(), items.size() * sizeof(ca_sim_item), hipMemcpyHostToDevice, call.stream), "hipMemcpyAsync of the items") &&
        call.note(hipStreamSynchronize(call.stream), "hipStreamSynchronize")) {   // (the copy has read the pageable list)
      o.n_items = (int64_t)items.size();
      call.timed([&]() { return launch_simulate(call.stream, o); });
    }
    items.clear();
    return call.rc == CA_OK;
  };
  for (int64_t n_lo = 0; n_lo < N; n_lo += NB) {
    const int64_t n_cnt = std::min<int64_t>(NB, N - n_lo);
    const size_t bytes = (size_t)n_cnt * G * sizeof(int32_t);
    if (!call.feed(U, clone, total, n_lo, n_cnt) || !call.note(hipMemsetAsync(o.Y, 0, bytes, call.stream), "hipMemsetAsync of the rows")) return call.failed();
    o.q0 = (uint64_t)(cell_offset + n_lo);
    for (int64_t li = 0; li < n_cnt; ++li)
      for (int64_t j = 0; j < total[n_lo + li]; j += CA_SIM_SEG) {
        items.push_back(ca_sim_item{(int32_t)li, (uint32_t)j});
        if ((int64_t)items.size() == max_items && !flush()) return call.failed();
      }
    if (!flush()) return call.failed();
    // the batch's rows to the caller, chunk by chunk through the two pinned buffers
    char* dst = reinterpret_cast<char*>(Y + (size_t)n_lo * G);
    const char* src = reinterpret_cast<const char*>(o.Y);
    const size_t nchunk = (bytes + chunk_bytes - 1) / chunk_bytes;
    for (size_t k = 0; k <= nchunk; ++k) {
      if (k < nchunk) {
        const size_t off = k * chunk_bytes, len = std::min(chunk_bytes, bytes - off);
        if (!call.ok(hipMemcpyAsync(stage[k & 1], src + off, len, hipMemcpyDeviceToHost, call.stream), "hipMemcpyAsync", len) ||
            !call.note(hipEventRecord(arrived[k & 1], call.stream), "hipEventRecord"))
          return call.failed();
      }
      if (k > 0) {
        const size_t off = (k - 1) * chunk_bytes, len = std::min(chunk_bytes, bytes - off);
        if (!call.note(hipEventSynchronize(arrived[(k - 1) & 1]), "hipEventSynchronize")) return call.failed();
        memcpy(dst + off, stage[(k - 1) & 1], len);
      }
    }
  }
  return call.done();
}
