// ca_eng_comm.inc -- part of clonealign_hip.hip (textually included there, in this order; one translation unit): C ABI, transports: setup sums over all ranks, RCCL communicator, one-shot peer-to-peer set-up (two-phase), benchmark, known-answer test, host callback.
namespace {
// the per-gene count totals are sums over ALL cells (SURVEY.md §8e): reduced once, when the transport is set
int setup_global_sums(ca_engine* h) {
  if (h->sums_global) return CA_OK;
  // a transport that died between the two reductions leaves colsum reduced and YtX not: no second transport may reduce colsum again
  if (h->sums_started) { h->err = "an earlier transport failed inside the setup reductions; this engine cannot take another one -- destroy it"; return CA_ERR_STATE; }
  h->sums_started = true;
  CACK(allreduce(h, h->colsum, h->G));
  if (h->P > 0 && h->K > 0) CACK(allreduce(h, h->YtX, (int64_t)h->G * h->P));
  SYNC(h);
  if (!h->mu_part.empty()) {
    // loc0 = NULL on a shard (ABI 6): mu_guess_g = mean over ALL cells of y_ng / rowMeans(Y)_n (R/inference-tflow.R:220-235) -- the ranks' partial sums and
    // cell counts are added here, then loc0 = safe_inverse_softplus(mu_guess) (:262, :6-11) exactly as create_impl does it for one handle
    const int G = h->G;
    std::vector<double> pack(h->mu_part);
    pack.push_back((double)h->N);
    HIPCK(h, hipMemcpyAsync(h->red, pack.data(), pack.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    CACK(allreduce(h, h->red, (int64_t)pack.size()));
    HIPCK(h, hipMemcpyAsync(pack.data(), h->red, pack.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    SYNC(h);
    std::vector<float> l0((size_t)G);
    for (int g = 0; g < G; ++g) {
      const double mu = pack[(size_t)g] / pack[(size_t)G];
      l0[g] = (float)(std::log(1.0 - std::exp(-std::fabs(mu))) + std::max(mu, 0.0));
    }
    CACK(upload_f(h, h->loc, l0));
    HIPCK(h, hipMemcpyAsync(h->loc_init, h->loc, (size_t)G * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    HIPCK(h, hipMemsetAsync(h->red, 0, pack.size() * sizeof(double), h->stream));
    CACK(refresh_derived(h));
    SYNC(h);
    h->mu_part.clear();
  }
  if (h->layout_series) {   // (this function runs when a transport has come up)
    // the ranks agree on the series form (its pick looks at the rank's own cell count): used where EVERY rank picked it; otherwise nobody uses it and everybody
    // goes back to the classic layout of the reduction buffer -- the collectives' lengths are then the same on all ranks either way
    double f[2] = {h->poly ? 1.0 : 0.0, 1.0};
    HIPCK(h, hipMemcpyAsync(h->red, f, sizeof(f), hipMemcpyHostToDevice, h->stream));
    SYNC(h);
    CACK(allreduce(h, h->red, 2));
    HIPCK(h, hipMemcpyAsync(f, h->red, sizeof(f), hipMemcpyDeviceToHost, h->stream));
    SYNC(h);
    HIPCK(h, hipMemsetAsync(h->red, 0, sizeof(f), h->stream));
    if (f[0] != f[1]) h->poly = false;
    if (!h->poly) {
      h->layout_series = false;
      h->off_g = 3 + h->C;
      h->off_y = h->off_g + (int64_t)h->G * (h->S + h->D);
      h->red_n = h->off_y + (int64_t)h->G * h->K;   // (the buffer is longer than this layout needs: the Gp - G padding rows of Y^T psi fit behind it)
      h->off_q = h->off_x = 0;
    }
    SYNC(h);
  }
  h->sums_global = true;
  return CA_OK;
}
}  // namespace

int ca_comm_unique_id(char id[128]) {
  if (!g_rccl.load()) { g_last_error = g_rccl.err; return CA_ERR_COMM; }
  ca_nccl_uid u;
  int rc = g_rccl.GetUniqueId(&u);
  if (rc != 0) { g_last_error = "ncclGetUniqueId failed"; return CA_ERR_COMM; }
  memcpy(id, u.internal, 128);
  return CA_OK;
}

int ca_comm_init(ca_handle h, const char id[128]) {
  if (!h || !id) return CA_ERR_INVALID;
  CA_NOT_IN_RUN(h);
  CACK(comm_check(h));   // a peer-to-peer transport that timed out leaves the engine dead: no falling back on the same handle
  if (!g_rccl.load()) { h->err = g_rccl.err; return CA_ERR_COMM; }
  HIPCK(h, hipSetDevice(h->device));
  ca_nccl_uid u;
  memcpy(u.internal, id, 128);
  int rc = g_rccl.CommInitRank(&h->comm, h->opt.world, u, h->opt.rank);
  if (rc != 0) {
    h->err = std::string("ncclCommInitRank: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "error");
    h->comm = nullptr;
    return CA_ERR_COMM;
  }
  return setup_global_sums(h);
}

int ca_p2p_export(ca_handle h, char handle[CA_P2P_HANDLE_BYTES]) {
  if (!h || !handle) return CA_ERR_INVALID;
  CA_NOT_IN_RUN(h);
  HIPCK(h, hipSetDevice(h->device));
  if (h->opt.world > CA_TB) { h->err = "peer-to-peer transport: at most " + std::to_string(CA_TB) + " ranks (one flag lane per rank)"; return CA_ERR_COMM; }
  if (!h->p2p) {
    ca_p2p* pp = new ca_p2p();
    const int W = h->opt.world;
    // room for everything one call reduces: the train pass's summands, the setup sums, the PCA / correlation packs
    pp->cap = std::max<int64_t>(std::max<int64_t>(h->red_n, (int64_t)h->G * (h->C + 2) + 64), 4096);
    pp->slab_bytes = (size_t)2 * W * pp->cap * 16;   // [parity 2][source W][cap] entries of 16 bytes: two halves of a double, each with the call's tag (k_p2p_allreduce)
    // Fine-grained memory or nothing: the slab is written by remote peers over xGMI and polled here, which ordinary
    // (coarse-grained) device memory does not keep coherent -- a stale flag would be a hang or a wrong sum.  The caller moves
    // on to RCCL when this fails.
    if (hipExtMallocWithFlags((void**)&pp->slab, pp->slab_bytes, hipDeviceMallocFinegrained) != hipSuccess) {
      (void)hipGetLastError();
      delete pp;
      h->err = "peer-to-peer transport: fine-grained device memory unavailable (hipExtMallocWithFlags(hipDeviceMallocFinegrained) failed)";
      return CA_ERR_COMM;
    }
    auto fail = [&](const std::string& m) { if (pp->err_host) hipHostFree(pp->err_host); if (pp->err_local) hipFree(pp->err_local); if (pp->peers_dev) hipFree(pp->peers_dev);
                                            hipFree(pp->slab); delete pp; h->err = m; return CA_ERR_HIP; };
    if (hipMemset(pp->slab, 0, pp->slab_bytes) != hipSuccess) return fail("hipMemset of the p2p slab failed");
    if (hipMalloc((void**)&pp->peers_dev, (size_t)W * sizeof(double*)) != hipSuccess) return fail("hipMalloc (p2p peer table) failed");
    if (hipMalloc((void**)&pp->err_local, sizeof(unsigned int)) != hipSuccess) return fail("hipMalloc (p2p error flag) failed");
    if (hipMemset(pp->err_local, 0, sizeof(unsigned int)) != hipSuccess) return fail("hipMemset (p2p error flag) failed");
    if (hipDeviceSynchronize() != hipSuccess) return fail("hipDeviceSynchronize (p2p setup) failed");   // (NULL-stream memsets are not ordered against the engine's non-blocking stream)
    if (hipHostMalloc((void**)&pp->err_host, sizeof(unsigned long long), hipHostMallocMapped) != hipSuccess) return fail("hipHostMalloc (p2p error word) failed");
    *pp->err_host = 0ull;
    if (hipHostGetDevicePointer((void**)&pp->err_dev, pp->err_host, 0) != hipSuccess) return fail("hipHostGetDevicePointer (p2p error word) failed");
    const int ms = h->opt.comm_timeout_ms > 0 ? h->opt.comm_timeout_ms : 10000;
    pp->timeout_ticks = (unsigned long long)((double)ms * 1000.0 * h->ticks_per_us);   // s_memrealtime ticks
    h->p2p = pp;
  }
  ca_p2p_wire w;
  memset(&w, 0, sizeof(w));
  HIPCK(h, hipIpcGetMemHandle(&w.mem, h->p2p->slab));
  w.cap = h->p2p->cap; w.rank = h->opt.rank; w.world = h->opt.world; w.device = h->device; w.pid = (int32_t)getpid();
  w.local_ptr = (uint64_t)(uintptr_t)h->p2p->slab;
  memset(handle, 0, CA_P2P_HANDLE_BYTES);
  memcpy(handle, &w, sizeof(w));
  return CA_OK;
}

static void p2p_unmap(ca_p2p* pp) {
  for (void*& q : pp->opened) if (q) { hipIpcCloseMemHandle(q); q = nullptr; }
  (void)hipGetLastError();
  pp->mapped = false;
}

// Phase 1: map every peer's slab.  Touches no peer and launches nothing, so a rank whose peer failed does not end up waiting for
// it: the caller agrees on every rank's result over its control plane and then calls ca_p2p_commit on all ranks.
int ca_p2p_connect(ca_handle h, const char* handles) {
  if (!h || !handles) return CA_ERR_INVALID;
  CA_NOT_IN_RUN(h);
  if (!h->p2p) { h->err = "ca_p2p_connect before ca_p2p_export"; return CA_ERR_STATE; }
  if (!variant_on(h, CA_VAR_P2P, "CA_P2P")) { h->err = "peer-to-peer transport switched off (CA_VAR_P2P)"; return CA_ERR_COMM; }
  HIPCK(h, hipSetDevice(h->device));
  ca_p2p* pp = h->p2p;
  if (pp->connected) { h->err = "ca_p2p_connect: the transport is already committed"; return CA_ERR_STATE; }
  const int W = h->opt.world;
  std::vector<double*> peers((size_t)W, nullptr);
  p2p_unmap(pp);
  pp->opened.assign((size_t)W, nullptr);
  auto fail = [&](const std::string& m) { p2p_unmap(pp); h->err = m; return CA_ERR_COMM; };
  for (int r = 0; r < W; ++r) {
    ca_p2p_wire w;
    memcpy(&w, handles + (size_t)r * CA_P2P_HANDLE_BYTES, sizeof(w));
    if (w.rank != r || w.world != W || w.cap != pp->cap)
      return fail("p2p handle " + std::to_string(r) + " does not match this problem (rank / world / payload size)");
    if (r == h->opt.rank) { peers[r] = pp->slab; continue; }
    if (w.device != h->device) {
      int can = 0;
      if (hipDeviceCanAccessPeer(&can, h->device, w.device) != hipSuccess || !can) {
        (void)hipGetLastError();
        return fail("no peer access from device " + std::to_string(h->device) + " to device " + std::to_string(w.device));
      }
      const hipError_t e = hipDeviceEnablePeerAccess(w.device, 0);
      (void)hipGetLastError();
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return fail(std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e));
    }
    if (w.pid == (int32_t)getpid()) {   // a handle of THIS process (one R session driving several devices): the slab's own address
      // ... but not two ranks of one process on ONE device: the runtime's device-wide synchronising calls (hipFree, hipMalloc of
      // a grown eps buffer, ...) made for one handle wait for every kernel on the device, also the other handle's all-reduce
      // kernel -- which waits for this rank.  Measured: the second all-reduce of such a pair ran into the device-side time
      // limit (tests/test_gpu_sharding.py).  Separate processes sharing a device are fine (their runtimes do not see each other).
      if (w.device == h->device && !(h->opt.variant_on & CA_VARX_P2P_SAME_DEVICE))
        return fail("peer-to-peer transport: ranks " + std::to_string(h->opt.rank) + " and " + std::to_string(r) + " are handles of one process on one "
                    "device; use one rank per device (or one process per rank)");
      peers[r] = (double*)(uintptr_t)w.local_ptr;
      continue;
    }
    void* q = nullptr;
    const hipError_t e = hipIpcOpenMemHandle(&q, w.mem, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return fail(std::string("hipIpcOpenMemHandle (rank ") + std::to_string(r) + "): " + hipGetErrorString(e));
    }
    pp->opened[r] = q;
    peers[r] = (double*)q;
  }
  if (hipMemcpy(pp->peers_dev, peers.data(), (size_t)W * sizeof(double*), hipMemcpyHostToDevice) != hipSuccess) return fail("hipMemcpy (p2p peer table) failed");
  pp->mapped = true;
  return CA_OK;
}

// Phase 2, collective: all_ranks_ok = 1 only if ca_p2p_connect returned CA_OK on EVERY rank (the caller's control plane says
// so).  Then the transport becomes the engine's all-reduce and the setup sums are reduced -- the first call that waits for
// peers.  all_ranks_ok = 0: the mappings are dropped and the engine is left without a transport (next: ca_comm_init).
int ca_p2p_commit(ca_handle h, int32_t all_ranks_ok) {
  if (!h) return CA_ERR_INVALID;
  CA_NOT_IN_RUN(h);
  if (!h->p2p) { h->err = "ca_p2p_commit before ca_p2p_export"; return CA_ERR_STATE; }
  HIPCK(h, hipSetDevice(h->device));
  ca_p2p* pp = h->p2p;
  if (!all_ranks_ok) { p2p_unmap(pp); pp->connected = false; return CA_OK; }
  if (!pp->mapped) { h->err = "ca_p2p_commit(1) without a successful ca_p2p_connect on this rank"; return CA_ERR_STATE; }
  pp->connected = true;
  return setup_global_sums(h);
}

// Times n_calls all-reduces of n_doubles doubles on one of the engine's device transports, back to back on the engine's stream
// (HIP events around the batch).  Collective: every rank calls it with the same arguments.  The buffer is scratch.
int ca_comm_benchmark(ca_handle h, int32_t transport, int32_t n_calls, int64_t n_doubles, double* us_per_call) {
  if (!h || !us_per_call || n_calls < 1 || n_doubles < 1) return CA_ERR_INVALID;
  CA_NOT_IN_RUN(h);
  HIPCK(h, hipSetDevice(h->device));
  const bool want_p2p = transport == CA_TRANSPORT_P2P;
  if (want_p2p && !(h->p2p && h->p2p->connected)) { h->err = "ca_comm_benchmark: no committed peer-to-peer transport"; return CA_ERR_STATE; }
  if (transport == CA_TRANSPORT_RCCL && !h->comm) { h->err = "ca_comm_benchmark: no RCCL communicator (ca_comm_init)"; return CA_ERR_STATE; }
  if (!want_p2p && transport != CA_TRANSPORT_RCCL) { h->err = "ca_comm_benchmark: transport must be CA_TRANSPORT_P2P or CA_TRANSPORT_RCCL"; return CA_ERR_INVALID; }
  double* buf = nullptr;
  HIPCK(h, hipMalloc((void**)&buf, (size_t)n_doubles * sizeof(double)));
  hipEvent_t e0 = nullptr, e1 = nullptr;
  auto cleanup = [&]() { if (e0) hipEventDestroy(e0); if (e1) hipEventDestroy(e1); hipFree(buf); };
  int rc = CA_OK;
  // the RCCL leg runs with the peer-to-peer transport hidden from allreduce()
  const bool was = h->p2p && h->p2p->connected;
  if (!want_p2p && was) h->p2p->connected = false;
  auto run = [&]() -> int {
    HIPCK(h, hipMemsetAsync(buf, 0, (size_t)n_doubles * sizeof(double), h->stream));
    HIPCK(h, hipEventCreate(&e0)); HIPCK(h, hipEventCreate(&e1));
    for (int i = 0; i < 3; ++i) CACK(allreduce(h, buf, n_doubles));   // warm-up (RCCL builds its channels on first use)
    HIPCK(h, hipEventRecord(e0, h->stream));
    for (int i = 0; i < n_calls; ++i) CACK(allreduce(h, buf, n_doubles));
    HIPCK(h, hipEventRecord(e1, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));
    CACK(comm_check(h));
    float ms = 0.f;
    HIPCK(h, hipEventElapsedTime(&ms, e0, e1));
    *us_per_call = (double)ms * 1e3 / n_calls;
    return CA_OK;
  };
  rc = run();
  if (!want_p2p && was) h->p2p->connected = true;
  cleanup();
  return rc;
}

int ca_comm_selftest(ca_handle h, int32_t n_rounds, int64_t n_doubles, int64_t* n_bad) {
  if (!h || !n_bad || n_rounds < 1 || n_doubles < 1) return CA_ERR_INVALID;
  CA_NOT_IN_RUN(h);
  HIPCK(h, hipSetDevice(h->device));
  *n_bad = 0;
  // Round 5 (ADVICE r4): the transport is asked what the loop asks of it, not six equal calls.  Call sizes ALTERNATE -- the train pass's
  // payload, a monitor pass's 3 + C doubles, and a vector longer than the peer-to-peer inbox (several pieces per call) -- in BURSTS of
  // back-to-back calls with no host synchronisation between them (both inbox parities and the sequence tags under the loop's own timing:
  // a fast rank one call ahead of a slow one), every sum checked; and, on the peer-to-peer transport, the RIDE form of the call (the
  // backward sweep's slabs folded and a block-partial sum added inside the all-reduce's launch, ca_p2p_args) against the same sums made
  // on the host.  Summands are small integers and halves times (rank + 1): every partial sum is exact in a double in any order.
  const double W = (double)std::max(h->opt.world, 1), tri = W * (W + 1.0) / 2.0;
  const bool p2p = h->p2p && h->p2p->connected;
  const int64_t big = p2p ? 2 * h->p2p->cap + 17 : 2 * n_doubles + 17;
  const int64_t sizes[3] = {n_doubles, std::min<int64_t>(n_doubles, 11), big};
  constexpr int BURST = 8;
  int64_t slot = 0;
  for (int64_t sz : sizes) slot = std::max(slot, sz);
  double* buf = nullptr;
  HIPCK(h, hipMalloc((void**)&buf, (size_t)(slot * BURST) * sizeof(double)));
  std::vector<double> host((size_t)(slot * BURST));
  auto pattern = [](int64_t i, int r) { return (double)((i * 7 + (int64_t)r * 13) % 251 + 1); };
  int64_t checked = 0;
  auto run = [&]() -> int {
    for (int r0 = 0; r0 < n_rounds; r0 += BURST) {
      const int nb = std::min(BURST, n_rounds - r0);
      for (int j = 0; j < nb; ++j) {
        const int r = r0 + j;
        const int64_t sz = sizes[r % 3];
        for (int64_t i = 0; i < sz; ++i) host[(size_t)(j * slot + i)] = (double)(h->opt.rank + 1) * pattern(i, r) + 0.5 * r;
      }
      HIPCK(h, hipMemcpyAsync(buf, host.data(), (size_t)(slot * nb) * sizeof(double), hipMemcpyHostToDevice, h->stream));
      for (int j = 0; j < nb; ++j) CACK(allreduce(h, buf + j * slot, sizes[(r0 + j) % 3]));     // back to back, no host in between
      HIPCK(h, hipMemcpyAsync(host.data(), buf, (size_t)(slot * nb) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      SYNC(h);
      for (int j = 0; j < nb; ++j) {
        const int r = r0 + j;
        const int64_t sz = sizes[r % 3];
        checked += sz;
        for (int64_t i = 0; i < sz; ++i)
          if (host[(size_t)(j * slot + i)] != tri * pattern(i, r) + W * 0.5 * r) *n_bad += 1;
      }
    }
    if (p2p && p2p_ride_ok(h, n_doubles) && n_doubles >= 8) {
      // ride form: entries [lo, lo + fn) are column sums of `ns` float slabs made here, entry `yi` also gets the sum of `ny` block partials
      const int64_t n = n_doubles, lo = std::min<int64_t>(3, n - 4), fn = n - lo - 1, yi = 0;
      const int ns = 5, ny = 37;
      std::vector<float> slabs((size_t)(ns * fn));
      std::vector<double> ywp((size_t)ny), base((size_t)n), want((size_t)n);
      for (int rep = 0; rep < 4; ++rep) {
        for (int sl = 0; sl < ns; ++sl) for (int64_t i = 0; i < fn; ++i) slabs[(size_t)(sl * fn + i)] = (float)((h->opt.rank + 1) * ((i + 3 * sl + rep) % 17));
        for (int b2 = 0; b2 < ny; ++b2) ywp[(size_t)b2] = (double)((h->opt.rank + 1) * ((b2 + rep) % 5)) * 0.5;
        for (int64_t i = 0; i < n; ++i) base[(size_t)i] = (double)(h->opt.rank + 1) * pattern(i, 100 + rep);
        for (int64_t i = 0; i < n; ++i) {   // what every rank contributes, then summed over ranks: (rank + 1) factors out -> tri
          double mine = (i >= lo && i < lo + fn) ? 0.0 : pattern(i, 100 + rep);
          if (i >= lo && i < lo + fn) for (int sl = 0; sl < ns; ++sl) mine += (double)(((i - lo) + 3 * sl + rep) % 17);
          if (i == yi) for (int b2 = 0; b2 < ny; ++b2) mine += 0.5 * (double)((b2 + rep) % 5);
          want[(size_t)i] = tri * mine;
        }
        float* gdev = nullptr; double* ydev = nullptr;
        HIPCK(h, hipMalloc((void**)&gdev, slabs.size() * sizeof(float)));
        if (hipMalloc((void**)&ydev, ywp.size() * sizeof(double)) != hipSuccess) { hipFree(gdev); h->err = "hipMalloc failed"; return CA_ERR_NOMEM; }
        hipMemcpyAsync(gdev, slabs.data(), slabs.size() * sizeof(float), hipMemcpyHostToDevice, h->stream);
        hipMemcpyAsync(ydev, ywp.data(), ywp.size() * sizeof(double), hipMemcpyHostToDevice, h->stream);
        hipMemcpyAsync(buf, base.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, h->stream);
        ca_ar_ride ride;
        ride.gpart = gdev; ride.nslice = ns; ride.fold_lo = lo; ride.fold_n = fn; ride.yw_part = ydev; ride.n_yw = ny; ride.yw_index = yi;
        int rc2 = allreduce(h, buf, n, &ride);
        if (rc2 == CA_OK && hipMemcpyAsync(host.data(), buf, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream) != hipSuccess) rc2 = CA_ERR_HIP;
        const hipError_t e2 = hipStreamSynchronize(h->stream);
        hipFree(gdev); hipFree(ydev);
        if (rc2 != CA_OK) return rc2;
        if (e2 != hipSuccess) { h->err = hipGetErrorString(e2); return CA_ERR_HIP; }
        CACK(comm_check(h));
        checked += n;
        for (int64_t i = 0; i < n; ++i) if (host[(size_t)i] != want[(size_t)i]) *n_bad += 1;
      }
    }
    return CA_OK;
  };
  const int rc = run();
  hipFree(buf);
  if (rc == CA_OK && *n_bad) h->err = "all-reduce known-answer test: " + std::to_string(*n_bad) + " of " + std::to_string(checked) + " sums are wrong";
  return rc;
}

int ca_set_host_allreduce(ca_handle h, ca_host_allreduce_fn fn, void* user) {
  if (!h || !fn) return CA_ERR_INVALID;
  CA_NOT_IN_RUN(h);
  CACK(comm_check(h));
  HIPCK(h, hipSetDevice(h->device));
  h->host_ar = fn;
  h->host_ar_user = user;
  return setup_global_sums(h);
}

