// ca_eng_ingest.inc -- part of clonealign_hip.hip (textually included there, in this order; one translation unit): ingestion: storage scan and conversion, selection gather, host -> device pipeline (float64 narrowed on the host), fit constants.

// storage pick from the scan of the (selected) counts -- the one rule of both ingest paths (upload_y / upload_y_sparse): sets ystore,
// ybytes, VEC, nseg, Gp, y_dev_bytes.  total = N * G of the selection (implicit zeros of a sparse matrix are counts too).
int pick_ystore(ca_engine* h, double mx, int fl, unsigned long long n255, int64_t total) {
  if (fl & 2) { h->err = "count matrix has negative or NaN entries"; return CA_ERR_INVALID; }
  int store = h->opt.y_storage;
  const bool integral = !(fl & 1);
  // u8 also serves matrices with a few entries above 255 (at most 1 in 64, each < 2^24): those keep 255 in
  // the dense byte and their excess in a sorted overflow list
  const bool u8_ok = integral && mx < 16777216.0 && (int64_t)n255 * 64 <= total;
  if (store == CA_YSTORE_AUTO) {
    if (!integral) store = CA_YSTORE_F32;
    else if (u8_ok) store = CA_YSTORE_U8;
    else if (mx <= 65535.0) store = CA_YSTORE_U16;
    else store = CA_YSTORE_F32;
  }
  if ((store == CA_YSTORE_U8 && !(integral && mx < 16777216.0)) || (store == CA_YSTORE_U16 && (!integral || mx > 65535.0))) {
    h->err = "requested y_storage cannot hold the counts (max " + std::to_string(mx) + ")";
    return CA_ERR_INVALID;
  }
  h->ystore = store;
  h->ybytes = store == CA_YSTORE_U8 ? 1 : store == CA_YSTORE_U16 ? 2 : 4;
  h->VEC = 16 / h->ybytes;
  const int segw = 64 * h->VEC;
  h->nseg = cdiv(h->G, segw);
  h->Gp = h->nseg * segw;
  h->y_dev_bytes = h->N * (int64_t)h->Gp * h->ybytes;
  // Kernels that take one thread per 16 BYTES of the resident matrix (k_bias_y, the tilers) use one-dimensional grids: 2^32 work-items = 64 GiB of matrix,
  // more than a quarter of this device's memory in ONE matrix (there are two copies).  Refuse instead of wrapping.
  if ((h->N * (int64_t)h->Gp) / 16 >= ((int64_t)1 << 32) || h->N >= ((int64_t)1 << 31)) {
    h->err = "count matrix too large for this build (cells x padded genes >= 2^36 bytes, or 2^31 cells)";
    return CA_ERR_INVALID;
  }
  return CA_OK;
}

// the u8 overflow list (h_orow / h_ocol / h_oval, n_ovf entries in the order the conversion appended them) into its fixed form:
// sorted by (cell, gene) for the CSR copy and by (gene, cell) for the CSC copy, 256-entry chunks per gene, all uploaded
int finish_ovf(ca_engine* h) {
  {
    const int64_t nz = h->n_ovf;
    std::vector<int64_t> idx(nz);
    for (int64_t i = 0; i < nz; ++i) idx[i] = i;
    std::sort(idx.begin(), idx.end(), [&](int64_t a, int64_t b) {
      return h->h_orow[a] != h->h_orow[b] ? h->h_orow[a] < h->h_orow[b] : h->h_ocol[a] < h->h_ocol[b]; });
    std::vector<int> r1(nz), c1(nz); std::vector<float> v1(nz);
    for (int64_t i = 0; i < nz; ++i) { r1[i] = h->h_orow[idx[i]]; c1[i] = h->h_ocol[idx[i]]; v1[i] = h->h_oval[idx[i]]; }
    h->h_orow = r1; h->h_ocol = c1; h->h_oval = v1;
    std::vector<int64_t> rowptr(h->N + 1, 0), colptr(h->G + 1, 0);
    for (int64_t i = 0; i < nz; ++i) { rowptr[r1[i] + 1]++; colptr[c1[i] + 1]++; }
    for (int64_t i = 0; i < h->N; ++i) rowptr[i + 1] += rowptr[i];
    for (int g = 0; g < h->G; ++g) colptr[g + 1] += colptr[g];
    std::vector<int> r2(nz); std::vector<float> v2(nz);
    {
      std::vector<int64_t> fill(colptr.begin(), colptr.end() - 1);
      for (int64_t i = 0; i < nz; ++i) { const int64_t q = fill[c1[i]]++; r2[q] = r1[i]; v2[q] = v1[i]; }   // rows ascending within a gene
    }
    // chunks of <= 256 entries inside each gene's CSC range
    std::vector<int64_t> chunk_start; std::vector<int> col_chunk_ptr(h->G + 1, 0);
    for (int g = 0; g < h->G; ++g) {
      col_chunk_ptr[g] = (int)chunk_start.size();
      for (int64_t e = colptr[g]; e < colptr[g + 1]; e += 256) chunk_start.push_back(e);
    }
    col_chunk_ptr[h->G] = (int)chunk_start.size();
    h->n_ovf_chunk = (int)chunk_start.size();
    chunk_start.push_back(nz);
    CACK(dalloc(h, &h->ovf_rowptr, h->N + 1));
    CACK(dalloc(h, &h->ovf_chunk_start, (int64_t)chunk_start.size()));
    CACK(dalloc(h, &h->ovf_col_chunk_ptr, h->G + 1));
    CACK(dalloc(h, &h->ovf_csum, (int64_t)h->n_ovf_chunk * std::max(h->K, 1)));
    HIPCK(h, hipMemcpyAsync(h->ovf_chunk_start, chunk_start.data(), chunk_start.size() * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    HIPCK(h, hipMemcpyAsync(h->ovf_col_chunk_ptr, col_chunk_ptr.data(), col_chunk_ptr.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    CACK(dalloc(h, &h->ovf_col, nz)); CACK(dalloc(h, &h->ovf_row2, nz));
    CACK(dalloc(h, &h->ovf_val, nz)); CACK(dalloc(h, &h->ovf_val2, nz));
    HIPCK(h, hipMemcpyAsync(h->ovf_rowptr, rowptr.data(), rowptr.size() * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    HIPCK(h, hipMemcpyAsync(h->ovf_col, c1.data(), nz * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCK(h, hipMemcpyAsync(h->ovf_row2, r2.data(), nz * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCK(h, hipMemcpyAsync(h->ovf_val, v1.data(), nz * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIPCK(h, hipMemcpyAsync(h->ovf_val2, v2.data(), nz * sizeof(float), hipMemcpyHostToDevice, h->stream));
    SYNC(h);   // (the sources are this function's vectors; and every copy above is ordered on the engine's stream, behind the buffers' zeroing)
  }
  return CA_OK;
}

template <typename ST>
int scan_and_convert(ca_engine* h, const ST* src_dev, int64_t sn, int64_t sg) {
  double* maxv = nullptr;
  int* flags = nullptr;
  HIPCK(h, hipMalloc((void**)&maxv, 32));
  flags = (int*)(maxv + 1);
  unsigned long long* cnt = (unsigned long long*)(maxv + 2);
  HIPCK(h, hipMemsetAsync(maxv, 0, 32, h->stream));
  const int64_t total = h->N * (int64_t)h->G;
  hipLaunchKernelGGL((k_scan_y<ST>), dim3(std::min<int64_t>(4096, cdiv(total, CA_TB))), dim3(CA_TB), 0, h->stream, src_dev, total, maxv, flags, cnt);
  HIPCK(h, hipGetLastError());
  double hm[4];
  HIPCK(h, hipMemcpyAsync(hm, maxv, 32, hipMemcpyDeviceToHost, h->stream));
  SYNC(h);
  const double mx = hm[0];
  int fl;
  memcpy(&fl, &hm[1], sizeof(int));
  unsigned long long n255;
  memcpy(&n255, &hm[2], sizeof(n255));
  {
    const int rcp = pick_ystore(h, mx, fl, n255, total);
    if (rcp != CA_OK) { hipFree(maxv); return rcp; }
  }
  const int store = h->ystore;
  uint8_t* yb = nullptr;
  CACK(dalloc(h, &yb, h->y_dev_bytes));
  h->Y = yb;
  HIPCK(h, hipMemsetAsync(maxv, 0, 32, h->stream));
  const int64_t tot = h->N * (int64_t)h->Gp;
  const dim3 grid = ca_grid_flat(tot, CA_TB);
  if (store == CA_YSTORE_U8 && n255 > 0) {
    h->n_ovf = (int64_t)n255;
    int *orow = nullptr, *ocol = nullptr; float* oval = nullptr;
    HIPCK(h, hipMalloc((void**)&orow, n255 * sizeof(int)));
    HIPCK(h, hipMalloc((void**)&ocol, n255 * sizeof(int)));
    HIPCK(h, hipMalloc((void**)&oval, n255 * sizeof(float)));
    hipLaunchKernelGGL((k_convert_y_u8ovf<ST>), grid, dim3(CA_TB), 0, h->stream, src_dev, (uint8_t*)h->Y, h->N, h->G, h->Gp, sn, sg, cnt, orow, ocol, oval);
    HIPCK(h, hipGetLastError());
    h->h_orow.resize(n255); h->h_ocol.resize(n255); h->h_oval.resize(n255);
    HIPCK(h, hipMemcpyAsync(h->h_orow.data(), orow, n255 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipMemcpyAsync(h->h_ocol.data(), ocol, n255 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipMemcpyAsync(h->h_oval.data(), oval, n255 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    SYNC(h);
    hipFree(orow); hipFree(ocol); hipFree(oval); hipFree(maxv);
    return finish_ovf(h);
  }
  if (store == CA_YSTORE_U8) hipLaunchKernelGGL((k_convert_y<ST, uint8_t>), grid, dim3(CA_TB), 0, h->stream, src_dev, (uint8_t*)h->Y, h->N, h->G, h->Gp, sn, sg, flags);
  else if (store == CA_YSTORE_U16) hipLaunchKernelGGL((k_convert_y<ST, uint16_t>), grid, dim3(CA_TB), 0, h->stream, src_dev, (uint16_t*)h->Y, h->N, h->G, h->Gp, sn, sg, flags);
  else hipLaunchKernelGGL((k_convert_y<ST, float>), grid, dim3(CA_TB), 0, h->stream, src_dev, (float*)h->Y, h->N, h->G, h->Gp, sn, sg, flags);
  HIPCK(h, hipGetLastError());
  HIPCK(h, hipMemcpyAsync(hm, maxv, 16, hipMemcpyDeviceToHost, h->stream));
  SYNC(h);
  memcpy(&fl, &hm[1], sizeof(int));
  hipFree(maxv);
  if (fl & 1) { h->err = "counts are not exactly representable in the on-device storage type"; return CA_ERR_INVALID; }
  return CA_OK;
}

template <typename ST>
int gather_y(ca_engine* h, const void* src, void** dst, int64_t sn, int64_t sg, const int64_t* ci_dev, const int32_t* gi_dev) {
  const int64_t total = h->N * (int64_t)h->G;
  HIPCK(h, hipMalloc(dst, (size_t)total * sizeof(ST)));
  hipLaunchKernelGGL((k_gather_y<ST>), ca_grid_flat(total, CA_TB), dim3(CA_TB), 0, h->stream, (const ST*)src, (ST*)*dst, h->N, h->G, sn, sg,
                     ci_dev, gi_dev);
  HIPCK(h, hipGetLastError());
  SYNC(h);
  return CA_OK;
}

// ---- host -> device ingestion (round 5; profiles/r05_ingest.txt) --------------------------------------------------------------
// The caller's matrix arrives in pageable host memory: from R an N x G column-major DOUBLE matrix (R/clonealign.R:212-222), 4 GB at
// 100k x 5k.  Until round 4 it went up as ONE pageable hipMemcpy into an N*G*8-byte device staging buffer (measured: 70 ms = the PCIe
// time of 4 GB, the whole fit that follows takes 60 ms).  Doubles carry nothing the engine can store -- its widest storage is float32
// and a count that is not exactly a float is an error either way -- so the bytes are narrowed on the HOST, on their way into the pinned
// buffers a copy has to pass through anyway: a few worker threads convert chunk c + 1 (float64 -> float32, every value checked for
// exactness) into one pinned buffer while the DMA engine moves chunk c out of the other.  Half the PCIe bytes, half the device
// staging, and the device sees exactly the values it saw before (the scan / conversion kernels and their results are unchanged).
// Other source types have nothing to narrow and keep the runtime's own pageable copy, which runs at 98 % of the pinned rate on these boxes
// (56.5 against 57.6 GB/s; the same bytes through this pipeline's memcpy threads measured SLOWER, 44 GB/s: profiles/r05_ingest.txt).
struct ingest_result { bool inexact = false; };
static int ingest_host_matrix(hipStream_t stream, std::string& err, const void* src, int64_t total, int src_dtype, void* dst_dev, ingest_result* res,
                              int64_t seg_len = 0, int64_t src_ld = 0) {
  // seg_len / src_ld (ABI 6, ca_problem.y_ld): the source is `total / seg_len` runs of seg_len contiguous elements, src_ld elements apart (a block of
  // rows of a column-major matrix); the device copy is compact.  0 = one dense run.
  if (seg_len <= 0 || src_ld == seg_len) { seg_len = total; src_ld = total; }
  const bool narrow = src_dtype == CA_F64;
  const size_t esz = src_dtype == CA_F64 ? 8 : (src_dtype == CA_F32 || src_dtype == CA_I32) ? 4 : src_dtype == CA_U16 ? 2 : 1;
  const size_t dsz = narrow ? 4 : esz;
  // 16 MiB of staged bytes per chunk, three pinned buffers, eight threads: measured on the MI355X boxes (256 host threads), tools/ingest_sweep.py --
  // 4 ... 24 threads are level (the loop runs at 85-90 % of the PCIe time of the narrowed bytes; 32+ threads and 64 MiB chunks lose to
  // pinning cost and scheduling noise, 4 MiB chunks to per-chunk overhead)
  const int64_t chunk_elems = (int64_t)(16u << 20) / (int64_t)dsz;
  const int64_t nchunks = (total + chunk_elems - 1) / chunk_elems;
  const int hw = (int)std::thread::hardware_concurrency();
  const int T = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(8, std::max(1, hw / 4)), (total + (1 << 18) - 1) >> 18));
  constexpr int NBMAX = 4;
  const int NB = (int)std::min<int64_t>(3, std::max<int64_t>(nchunks, 2));
  void* pin[NBMAX] = {};
  hipEvent_t ev[NBMAX] = {};
  auto fail = [&](const char* what, hipError_t e) { err = std::string(what) + ": " + hipGetErrorString(e); return CA_ERR_HIP; };
  hipError_t e = hipSuccess;
  {   // ONE pinned allocation for all buffers (pinning costs ~0.1 ms per MiB plus a fixed cost per call)
    void* base = nullptr;
    const size_t one = (size_t)std::min<int64_t>(chunk_elems, total) * dsz;
    e = hipHostMalloc(&base, one * NB);
    for (int b = 0; b < NB && e == hipSuccess; ++b) { pin[b] = reinterpret_cast<char*>(base) + one * b; e = hipEventCreateWithFlags(&ev[b], hipEventDisableTiming); }
  }
  std::atomic<int64_t> free_for[NBMAX];   // the chunk that may now be written into pinned buffer b
  for (int b = 0; b < NBMAX; ++b) free_for[b].store(b);
  std::vector<std::atomic<int>> filled((size_t)nchunks);
  for (auto& f : filled) f.store(0);
  std::atomic<int> inexact{0}, abort_all{0};
  auto fill_slice = [&](int64_t c, int t) {
    const int b = (int)(c % NB);
    const int64_t e0 = c * chunk_elems, n = std::min<int64_t>(chunk_elems, total - e0);
    // slice t of the chunk (multiples of 4096 elements: whole pages of the source, so the threads' pieces do not share lines)
    const int64_t per = ((n + T - 1) / T + 4095) & ~(int64_t)4095;
    const int64_t a = std::min<int64_t>(n, (int64_t)t * per), z = std::min<int64_t>(n, a + per);
    int bad = 0;
    for (int64_t i = a; i < z;) {   // run by run of the source (one run when it is dense)
      const int64_t lin = e0 + i, seg = lin / seg_len, off = lin - seg * seg_len, m = std::min<int64_t>(z - i, seg_len - off);
      const int64_t s0 = seg * src_ld + off;
      if (narrow) {
        const double* sp = reinterpret_cast<const double*>(src) + s0;
        float* dp = reinterpret_cast<float*>(pin[b]) + i;
        for (int64_t j = 0; j < m; ++j) { const double v = sp[j]; const float f = (float)v; dp[j] = f; bad |= ((double)f != v); }   // (NaN flags itself)
      } else {
        memcpy(reinterpret_cast<char*>(pin[b]) + (size_t)i * esz, reinterpret_cast<const char*>(src) + (size_t)s0 * esz, (size_t)m * esz);
      }
      i += m;
    }
    if (bad) inexact.store(1, std::memory_order_relaxed);
    filled[(size_t)c].fetch_add(1, std::memory_order_release);
  };
  auto worker = [&](int t) {
    for (int64_t c = 0; c < nchunks; ++c) {
      while (free_for[c % NB].load(std::memory_order_acquire) < c) { if (abort_all.load(std::memory_order_relaxed)) return; std::this_thread::yield(); }
      fill_slice(c, t);
    }
  };
  std::vector<std::thread> pool;
  if (e == hipSuccess) {
    try { for (int t = 1; t < T; ++t) pool.emplace_back(worker, t); }
    catch (...) {   // thread limit of a restricted container: a std::system_error must not cross the C ABI (ADVICE r5) -- stop cleanly
      abort_all.store(1);
      for (auto& th : pool) th.join();
      for (int b = 0; b < NB; ++b) if (ev[b]) hipEventDestroy(ev[b]);
      if (pin[0]) hipHostFree(pin[0]);
      err = "upload of the count matrix: cannot start the host conversion threads";
      return CA_ERR_NOMEM;
    }
  }
  int rc = CA_OK;
  if (e != hipSuccess) rc = fail("pinned staging buffers of the count matrix", e);
  // this thread is worker 0 of every chunk and the one that queues the copies; the other workers run ahead into the free buffers
  for (int64_t c = 0; c < nchunks && rc == CA_OK; ++c) {
    const int b = (int)(c % NB);
    const int64_t e0 = c * chunk_elems, n = std::min<int64_t>(chunk_elems, total - e0);
    fill_slice(c, 0);   // (free_for[b] >= c holds: this thread released it, below)
    while (filled[(size_t)c].load(std::memory_order_acquire) < T) std::this_thread::yield();
    e = hipMemcpyAsync(reinterpret_cast<char*>(dst_dev) + (size_t)e0 * dsz, pin[b], (size_t)n * dsz, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipEventRecord(ev[b], stream);
    // the buffer that chunk c + 1 wants held chunk c + 1 - NB: once THAT copy is done it is free (the copies queued since run meanwhile)
    const int64_t prev = c + 1 - NB;
    if (e == hipSuccess && prev >= 0) e = hipEventSynchronize(ev[prev % NB]);
    if (e != hipSuccess) { rc = fail("upload of the count matrix", e); break; }
    if (prev >= 0) free_for[prev % NB].store(c + 1, std::memory_order_release);
  }
  if (rc != CA_OK) abort_all.store(1);
  for (auto& th : pool) th.join();
  if (rc == CA_OK) { e = hipStreamSynchronize(stream); if (e != hipSuccess) rc = fail("upload of the count matrix", e); }
  for (int b = 0; b < NB; ++b) if (ev[b]) hipEventDestroy(ev[b]);
  if (pin[0]) hipHostFree(pin[0]);
  if (res) res->inexact = inexact.load() != 0;
  return rc;
}

int upload_y(ca_engine* h, const ca_problem* p) {
  // the caller's matrix: N_src x G_src when a selection is given (ca_problem.cell_index / gene_index), else N x G
  const bool sel = p->cell_index || p->gene_index;
  const int64_t Ns = sel ? p->N_src : h->N;
  const int64_t Gs = sel ? (int64_t)p->G_src : (int64_t)h->G;
  const int64_t total = Ns * Gs;
  size_t esz = p->y_dtype == CA_F64 ? 8 : (p->y_dtype == CA_F32 || p->y_dtype == CA_I32) ? 4 : p->y_dtype == CA_U16 ? 2 : 1;
  // ABI 6: the source may be a block of a larger matrix (ca_problem.y_ld): `nrun` runs of `run` contiguous counts, `ld` counts apart
  const int64_t run = p->layout == CA_COL_MAJOR ? Ns : Gs, nrun = p->layout == CA_COL_MAJOR ? Gs : Ns;
  const int64_t ld = p->y_ld > 0 ? p->y_ld : run;
  if (ld < run) { h->err = "y_ld is smaller than the matrix it strides over"; return CA_ERR_INVALID; }
  const void* src = p->Y;
  void* staging = nullptr;
  void* cut = nullptr;
  int64_t* ci_dev = nullptr; int32_t* gi_dev = nullptr;
  auto cleanup = [&]() { if (staging) hipFree(staging); if (cut) hipFree(cut); if (ci_dev) hipFree(ci_dev); if (gi_dev) hipFree(gi_dev); };
  int y_dtype = p->y_dtype;   // of `src` as the kernels below see it
  if (!p->y_on_device) {
    // chunked through pinned double buffers, float64 narrowed to float32 on the way (ingest_host_matrix): the device staging is the
    // source's layout at <= 4 bytes per count
    if (y_dtype == CA_F64) esz = 4;
    {
      const hipError_t e = hipMalloc(&staging, (size_t)total * esz);
      if (e != hipSuccess) { h->err = std::string("hipMalloc of ") + std::to_string((size_t)total * esz) + " bytes (count matrix staging): " + hipGetErrorString(e); return CA_ERR_NOMEM; }
    }
    ingest_result ir;
    if (p->y_dtype == CA_F64) {
      int rci;
      try { rci = ingest_host_matrix(h->stream, h->err, p->Y, total, p->y_dtype, staging, &ir, run, ld); }
      catch (const std::exception& ex) { h->err = std::string("upload of the count matrix: ") + ex.what(); rci = CA_ERR_NOMEM; }   // (nothing unwinds through the C ABI)
      if (rci != CA_OK) { cleanup(); return rci; }
    } else if ((ld == run ? hipMemcpy(staging, p->Y, (size_t)total * esz, hipMemcpyHostToDevice)
                          : hipMemcpy2D(staging, (size_t)run * esz, p->Y, (size_t)ld * esz, (size_t)run * esz, (size_t)nrun, hipMemcpyHostToDevice)) != hipSuccess) {
      cleanup(); h->err = "upload of the count matrix failed"; return CA_ERR_HIP;
    }
    if (p->y_dtype == CA_F64) y_dtype = CA_F32;
    if (ir.inexact && sel) {
      // some double of the RAW matrix is not a float, but it may lie outside the selection (which is all the fit may judge): take the
      // matrix up again as it is, 8 bytes per count, and let the gather below cut it first -- the rare path
      hipFree(staging); staging = nullptr;
      const hipError_t e = hipMalloc(&staging, (size_t)total * 8);
      if (e != hipSuccess) { cleanup(); h->err = std::string("hipMalloc of the count matrix staging: ") + hipGetErrorString(e); return CA_ERR_NOMEM; }
      if ((ld == run ? hipMemcpy(staging, p->Y, (size_t)total * 8, hipMemcpyHostToDevice)
                     : hipMemcpy2D(staging, (size_t)run * 8, p->Y, (size_t)ld * 8, (size_t)run * 8, (size_t)nrun, hipMemcpyHostToDevice)) != hipSuccess) {
        cleanup(); h->err = "upload of the count matrix failed"; return CA_ERR_HIP;
      }
      y_dtype = CA_F64;
    } else if (ir.inexact) {
      // a double that is not exactly a float can only be an error: NaN / negative takes precedence, as in the scan below
      double* maxv = nullptr;
      if (hipMalloc((void**)&maxv, 32) != hipSuccess) { cleanup(); h->err = "hipMalloc failed"; return CA_ERR_NOMEM; }
      double hm[4] = {0, 0, 0, 0};
      hipMemsetAsync(maxv, 0, 32, h->stream);
      hipLaunchKernelGGL((k_scan_y<float>), dim3(std::min<int64_t>(4096, cdiv(total, CA_TB))), dim3(CA_TB), 0, h->stream, (const float*)staging, total, maxv,
                         (int*)(maxv + 1), (unsigned long long*)(maxv + 2));
      hipMemcpyAsync(hm, maxv, 32, hipMemcpyDeviceToHost, h->stream);
      const hipError_t e = hipStreamSynchronize(h->stream);
      hipFree(maxv);
      cleanup();
      if (e != hipSuccess) { h->err = hipGetErrorString(e); return CA_ERR_HIP; }
      int fl;
      memcpy(&fl, &hm[1], sizeof(int));
      h->err = (fl & 2) ? "count matrix has negative or NaN entries" : "counts are not exactly representable in the on-device storage type";
      return CA_ERR_INVALID;
    }
    src = staging;
  }
  // strides of `src` as the kernels below see it: the staging copy of a host matrix is compact, a device matrix keeps its leading dimension
  const int64_t ldd = p->y_on_device ? ld : run;
  int64_t sn = p->layout == CA_COL_MAJOR ? 1 : ldd;
  int64_t sg = p->layout == CA_COL_MAJOR ? ldd : 1;
  int rc = CA_OK;
  if (sel || (p->y_on_device && ld != run)) {   // (a strided device block is compacted the same way: the scan below walks a dense matrix)
    // selection lists: validated on the host (strictly increasing, in range), applied by a device gather into a compact
    // row-major copy of the source type -- the storage scan / conversion below then sees only the selected counts
    auto bad = [&](const char* m) { cleanup(); h->err = m; return CA_ERR_INVALID; };
    if (p->cell_index) {
      for (int64_t n = 0; n < h->N; ++n)
        if (p->cell_index[n] < 0 || p->cell_index[n] >= Ns || (n > 0 && p->cell_index[n] <= p->cell_index[n - 1]))
          return bad("cell_index must be strictly increasing and within [0, N_src)");
      if (hipMalloc((void**)&ci_dev, (size_t)h->N * sizeof(int64_t)) != hipSuccess ||
          hipMemcpy(ci_dev, p->cell_index, (size_t)h->N * sizeof(int64_t), hipMemcpyHostToDevice) != hipSuccess) return bad("cell_index upload failed");
    } else if (h->N != Ns) return bad("N must equal N_src when cell_index is NULL");
    if (p->gene_index) {
      for (int g = 0; g < h->G; ++g)
        if (p->gene_index[g] < 0 || p->gene_index[g] >= Gs || (g > 0 && p->gene_index[g] <= p->gene_index[g - 1]))
          return bad("gene_index must be strictly increasing and within [0, G_src)");
      if (hipMalloc((void**)&gi_dev, (size_t)h->G * sizeof(int32_t)) != hipSuccess ||
          hipMemcpy(gi_dev, p->gene_index, (size_t)h->G * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) return bad("gene_index upload failed");
    } else if (h->G != Gs) return bad("G must equal G_src when gene_index is NULL");
    switch (y_dtype) {
      case CA_F64: rc = gather_y<double>(h, src, &cut, sn, sg, ci_dev, gi_dev); break;
      case CA_F32: rc = gather_y<float>(h, src, &cut, sn, sg, ci_dev, gi_dev); break;
      case CA_I32: rc = gather_y<int32_t>(h, src, &cut, sn, sg, ci_dev, gi_dev); break;
      case CA_U16: rc = gather_y<uint16_t>(h, src, &cut, sn, sg, ci_dev, gi_dev); break;
      case CA_U8: rc = gather_y<uint8_t>(h, src, &cut, sn, sg, ci_dev, gi_dev); break;
      default: h->err = "unknown y_dtype"; rc = CA_ERR_INVALID;
    }
    if (rc != CA_OK) { cleanup(); return rc; }
    if (staging) { hipFree(staging); staging = nullptr; }
    src = cut; sn = h->G; sg = 1;
  }
  switch (y_dtype) {
    case CA_F64: rc = scan_and_convert<double>(h, (const double*)src, sn, sg); break;
    case CA_F32: rc = scan_and_convert<float>(h, (const float*)src, sn, sg); break;
    case CA_I32: rc = scan_and_convert<int32_t>(h, (const int32_t*)src, sn, sg); break;
    case CA_U16: rc = scan_and_convert<uint16_t>(h, (const uint16_t*)src, sn, sg); break;
    case CA_U8: rc = scan_and_convert<uint8_t>(h, (const uint8_t*)src, sn, sg); break;
    default: h->err = "unknown y_dtype"; rc = CA_ERR_INVALID;
  }
  cleanup();
  return rc;
}

// ---- compressed count matrix (ca_create_sparse) ----------------------------------------------------------------------------------
// The caller's CSR / CSC arrays go up as they are (float64 values narrowed through ingest_host_matrix, as a dense float64 Y is); the
// device checks their canonical form, scans the SELECTED stored entries for the storage pick (pick_ystore, as the dense path), turns
// CSC into CSR over the selection, and expands each selected cell's run into its resident row (k_sp_densify).  No N x G buffer exists at
// any point: peak memory is the resident matrix plus the compressed arrays (plus the CSR transpose of a CSC matrix).
struct sp_bufs {   // device buffers owned by one upload_y_sparse call
  std::vector<void*> p;
  template <typename T> hipError_t alloc(T** out, int64_t n) {
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, (size_t)std::max<int64_t>(n, 1) * sizeof(T));
    if (e == hipSuccess) p.push_back(q);
    *out = (T*)q;
    return e;
  }
  void release(void* q) { for (auto& x : p) if (x == q) { hipFree(x); x = nullptr; } }
  ~sp_bufs() { for (void* x : p) if (x) hipFree(x); }
};
#define SPCK(h, x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) { (h)->err = std::string("sparse count matrix: ") + hipGetErrorString(e_); return e_ == hipErrorOutOfMemory ? CA_ERR_NOMEM : CA_ERR_HIP; } } while (0)

// scan, storage pick and densify of a CSR view over the selection (rows / ginv as in ca_k_sparse.hip.h); scratch = 32 zeroed bytes
template <typename PT, typename IT, typename VT>
int sparse_densify(ca_engine* h, sp_bufs& b, const PT* ptr, const IT* idx, const VT* val, const int64_t* rows, const int32_t* ginv, double* scratch) {
  int* flags = (int*)(scratch + 1);
  unsigned long long* cnt = (unsigned long long*)(scratch + 2);
  const int64_t total = h->N * (int64_t)h->G;
  hipLaunchKernelGGL((k_sp_scan<PT, IT, VT>), dim3((unsigned)std::min<int64_t>(4096, cdiv(h->N, CA_TB / 64))), dim3(CA_TB), 0, h->stream, ptr, idx, val,
                     rows, ginv, h->N, scratch, flags, cnt);
  HIPCK(h, hipGetLastError());
  double hm[4];
  HIPCK(h, hipMemcpyAsync(hm, scratch, 32, hipMemcpyDeviceToHost, h->stream));
  SYNC(h);
  int fl;
  memcpy(&fl, &hm[1], sizeof(int));
  unsigned long long n255;
  memcpy(&n255, &hm[2], sizeof(n255));
  CACK(pick_ystore(h, hm[0], fl, n255, total));
  uint8_t* yb = nullptr;
  CACK(dalloc(h, &yb, h->y_dev_bytes));
  h->Y = yb;
  HIPCK(h, hipMemsetAsync(scratch, 0, 32, h->stream));
  const bool ovf = h->ystore == CA_YSTORE_U8 && n255 > 0;
  int *orow = nullptr, *ocol = nullptr; float* oval = nullptr;
  if (ovf) {
    h->n_ovf = (int64_t)n255;
    SPCK(h, b.alloc(&orow, (int64_t)n255)); SPCK(h, b.alloc(&ocol, (int64_t)n255)); SPCK(h, b.alloc(&oval, (int64_t)n255));
  }
  const int seg = std::min(h->Gp, 32768 / h->ybytes);   // LDS budget of a row segment: 32 KiB (Gp * ybytes is a multiple of 1 KiB)
  hipLaunchKernelGGL((k_sp_densify<PT, IT, VT>), dim3((unsigned)h->N), dim3(CA_TB), (size_t)seg * h->ybytes, h->stream, ptr, idx, val, rows, ginv,
                     h->Gp, h->ybytes, seg, (uint8_t*)h->Y, flags, ovf ? cnt : nullptr, orow, ocol, oval);
  HIPCK(h, hipGetLastError());
  HIPCK(h, hipMemcpyAsync(hm, scratch, 32, hipMemcpyDeviceToHost, h->stream));
  SYNC(h);
  memcpy(&fl, &hm[1], sizeof(int));
  if (ovf) {
    h->h_orow.resize(n255); h->h_ocol.resize(n255); h->h_oval.resize(n255);
    HIPCK(h, hipMemcpyAsync(h->h_orow.data(), orow, n255 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipMemcpyAsync(h->h_ocol.data(), ocol, n255 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipMemcpyAsync(h->h_oval.data(), oval, n255 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    SYNC(h);
    return finish_ovf(h);
  }
  if (fl & 1) { h->err = "counts are not exactly representable in the on-device storage type"; return CA_ERR_INVALID; }
  return CA_OK;
}

template <typename IT, typename VT>
int sparse_ingest(ca_engine* h, sp_bufs& b, const ca_sparse* sp, const IT* ptr, const IT* idx, const VT* val, int64_t Ns, int64_t Gs,
                  const int64_t* ci_dev, const int32_t* gi_dev, double* scratch) {
  const bool csc = sp->kind == CA_SPARSE_CSC;
  const int64_t nrun = csc ? Gs : Ns, ndim = csc ? Ns : Gs, nnz = sp->nnz;
  int* flags = (int*)(scratch + 1);
  hipLaunchKernelGGL((k_sp_check<IT>), dim3((unsigned)std::min<int64_t>(4096, std::max<int64_t>(1, cdiv(nrun, CA_TB / 64)))), dim3(CA_TB), 0, h->stream,
                     ptr, idx, nrun, ndim, nnz, flags);
  HIPCK(h, hipGetLastError());
  int fl = 0;
  HIPCK(h, hipMemcpyAsync(&fl, flags, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  SYNC(h);
  if (fl & 4) { h->err = "sparse count matrix: ptr must start at 0, never decrease and end at nnz"; return CA_ERR_INVALID; }
  if (fl & 8) { h->err = std::string("sparse count matrix: an index is out of range (") + (csc ? "cell" : "gene") + " indices must lie in [0, " +
                         std::to_string(ndim) + "))"; return CA_ERR_INVALID; }
  if (fl & 16) { h->err = "sparse count matrix: indices must be strictly increasing within each run (unsorted or duplicate entries)"; return CA_ERR_INVALID; }
  HIPCK(h, hipMemsetAsync(scratch, 0, 32, h->stream));
  // inverse maps of the selection: source gene -> selected gene or -1 (and for CSC, source cell -> selected cell or -1)
  int32_t *ginv = nullptr, *cinv = nullptr;
  if (gi_dev) {
    SPCK(h, b.alloc(&ginv, Gs));
    HIPCK(h, hipMemsetAsync(ginv, 0xFF, (size_t)Gs * sizeof(int32_t), h->stream));
    hipLaunchKernelGGL((k_sp_inverse<int32_t>), dim3((unsigned)cdiv(h->G, CA_TB)), dim3(CA_TB), 0, h->stream, gi_dev, (int64_t)h->G, ginv);
    HIPCK(h, hipGetLastError());
  }
  if (!csc) return sparse_densify<IT, IT, VT>(h, b, ptr, idx, val, ci_dev, ginv, scratch);
  if (ci_dev) {
    SPCK(h, b.alloc(&cinv, Ns));
    HIPCK(h, hipMemsetAsync(cinv, 0xFF, (size_t)Ns * sizeof(int32_t), h->stream));
    hipLaunchKernelGGL((k_sp_inverse<int64_t>), dim3((unsigned)cdiv(h->N, CA_TB)), dim3(CA_TB), 0, h->stream, ci_dev, h->N, cinv);
    HIPCK(h, hipGetLastError());
  }
  // CSC -> CSR of the selection: per-cell counts, exclusive scan, scatter (genes already in the selection's numbering)
  int64_t* rowptr = nullptr; unsigned long long* fill = nullptr;
  SPCK(h, b.alloc(&rowptr, h->N + 1));
  SPCK(h, b.alloc(&fill, h->N));
  HIPCK(h, hipMemsetAsync(rowptr, 0, (size_t)(h->N + 1) * sizeof(int64_t), h->stream));
  const dim3 gw((unsigned)std::min<int64_t>(4096, std::max<int64_t>(1, cdiv(nrun, CA_TB / 64))));
  hipLaunchKernelGGL((k_sp_csc_count<IT>), gw, dim3(CA_TB), 0, h->stream, ptr, idx, nrun, ginv, cinv, (unsigned long long*)rowptr);
  HIPCK(h, hipGetLastError());
  hipLaunchKernelGGL(k_sp_exscan, dim3(1), dim3(1024), 0, h->stream, rowptr, h->N);
  HIPCK(h, hipGetLastError());
  int64_t nsel = 0;
  HIPCK(h, hipMemcpyAsync(&nsel, rowptr + h->N, sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
  HIPCK(h, hipMemcpyAsync(fill, rowptr, (size_t)h->N * sizeof(int64_t), hipMemcpyDeviceToDevice, h->stream));
  SYNC(h);
  int32_t* col = nullptr; VT* v2 = nullptr;
  SPCK(h, b.alloc(&col, nsel));
  SPCK(h, b.alloc(&v2, nsel));
  hipLaunchKernelGGL((k_sp_csc_scatter<IT, VT>), gw, dim3(CA_TB), 0, h->stream, ptr, idx, val, nrun, ginv, cinv, fill, col, v2);
  HIPCK(h, hipGetLastError());
  SYNC(h);
  b.release(fill); b.release(cinv); b.release(ginv);
  b.release((void*)ptr); b.release((void*)idx); b.release((void*)val);   // (the uploaded copies, if these are ours; the caller's device arrays are not in b)
  return sparse_densify<int64_t, int32_t, VT>(h, b, rowptr, col, v2, nullptr, nullptr, scratch);
}

int upload_y_sparse(ca_engine* h, const ca_problem* p, const ca_sparse* sp) {
  // the caller's matrix: N_src x G_src when a selection is given, else N x G (descriptor fields checked by ca_create_sparse)
  const bool sel = p->cell_index || p->gene_index;
  const int64_t Ns = sel ? p->N_src : h->N;
  const int64_t Gs = sel ? (int64_t)p->G_src : (int64_t)h->G;
  const bool csc = sp->kind == CA_SPARSE_CSC;
  const int64_t nrun = csc ? Gs : Ns, nnz = sp->nnz;
  const size_t ib = (size_t)sp->index_bytes;
  const size_t vsz = sp->val_dtype == CA_F64 ? 8 : (sp->val_dtype == CA_F32 || sp->val_dtype == CA_I32) ? 4 : sp->val_dtype == CA_U16 ? 2 : 1;
  sp_bufs b;
  auto bad = [&](const char* m) { h->err = m; return CA_ERR_INVALID; };
  // selection lists: validated on the host as on the dense path
  int64_t* ci_dev = nullptr; int32_t* gi_dev = nullptr;
  if (p->cell_index) {
    for (int64_t n = 0; n < h->N; ++n)
      if (p->cell_index[n] < 0 || p->cell_index[n] >= Ns || (n > 0 && p->cell_index[n] <= p->cell_index[n - 1]))
        return bad("cell_index must be strictly increasing and within [0, N_src)");
    SPCK(h, b.alloc(&ci_dev, h->N));
    SPCK(h, hipMemcpy(ci_dev, p->cell_index, (size_t)h->N * sizeof(int64_t), hipMemcpyHostToDevice));
  } else if (h->N != Ns) return bad("N must equal N_src when cell_index is NULL");
  if (p->gene_index) {
    for (int g = 0; g < h->G; ++g)
      if (p->gene_index[g] < 0 || p->gene_index[g] >= Gs || (g > 0 && p->gene_index[g] <= p->gene_index[g - 1]))
        return bad("gene_index must be strictly increasing and within [0, G_src)");
    SPCK(h, b.alloc(&gi_dev, h->G));
    SPCK(h, hipMemcpy(gi_dev, p->gene_index, (size_t)h->G * sizeof(int32_t), hipMemcpyHostToDevice));
  } else if (h->G != Gs) return bad("G must equal G_src when gene_index is NULL");
  // the compressed arrays on the device, each in its own dtype (float64 values narrowed to float32 when every value is a float)
  const void *dptr = sp->ptr, *didx = sp->idx, *dval = sp->val;
  int vdt = sp->val_dtype;
  if (!sp->on_device) {
    char *q = nullptr, *x = nullptr;
    SPCK(h, b.alloc(&q, (int64_t)((nrun + 1) * ib)));
    SPCK(h, hipMemcpy(q, sp->ptr, (size_t)(nrun + 1) * ib, hipMemcpyHostToDevice));
    SPCK(h, b.alloc(&x, (int64_t)(nnz * ib)));
    if (nnz > 0) SPCK(h, hipMemcpy(x, sp->idx, (size_t)nnz * ib, hipMemcpyHostToDevice));
    dptr = q; didx = x;
    char* v = nullptr;
    if (vdt == CA_F64 && nnz > 0) {
      SPCK(h, b.alloc(&v, nnz * 4));
      ingest_result ir;
      int rci;
      try { rci = ingest_host_matrix(h->stream, h->err, sp->val, nnz, CA_F64, v, &ir); }
      catch (const std::exception& ex) { h->err = std::string("upload of the count matrix: ") + ex.what(); rci = CA_ERR_NOMEM; }   // (nothing unwinds through the C ABI)
      if (rci != CA_OK) return rci;
      if (ir.inexact) {
        // some value is not a float (non-integral, NaN, huge, or outside the selection): up again as float64, the scan below judges it
        b.release(v);
        SPCK(h, b.alloc(&v, nnz * 8));
        SPCK(h, hipMemcpy(v, sp->val, (size_t)nnz * 8, hipMemcpyHostToDevice));
      } else {
        vdt = CA_F32;
      }
    } else {
      SPCK(h, b.alloc(&v, (int64_t)(nnz * vsz)));
      if (nnz > 0) SPCK(h, hipMemcpy(v, sp->val, (size_t)nnz * vsz, hipMemcpyHostToDevice));
    }
    dval = v;
  }
  double* scratch = nullptr;   // max, flags, count above 255
  SPCK(h, b.alloc(&scratch, 4));
  HIPCK(h, hipMemsetAsync(scratch, 0, 32, h->stream));
#define CA_SP_VT(IT)                                                                                                                       \
  switch (vdt) {                                                                                                                           \
    case CA_F64: return sparse_ingest<IT, double>(h, b, sp, (const IT*)dptr, (const IT*)didx, (const double*)dval, Ns, Gs, ci_dev, gi_dev, scratch);   \
    case CA_F32: return sparse_ingest<IT, float>(h, b, sp, (const IT*)dptr, (const IT*)didx, (const float*)dval, Ns, Gs, ci_dev, gi_dev, scratch);     \
    case CA_I32: return sparse_ingest<IT, int32_t>(h, b, sp, (const IT*)dptr, (const IT*)didx, (const int32_t*)dval, Ns, Gs, ci_dev, gi_dev, scratch); \
    case CA_U16: return sparse_ingest<IT, uint16_t>(h, b, sp, (const IT*)dptr, (const IT*)didx, (const uint16_t*)dval, Ns, Gs, ci_dev, gi_dev, scratch); \
    default: return sparse_ingest<IT, uint8_t>(h, b, sp, (const IT*)dptr, (const IT*)didx, (const uint8_t*)dval, Ns, Gs, ci_dev, gi_dev, scratch);   \
  }
  if (ib == 4) { CA_SP_VT(int32_t) }
  CA_SP_VT(int64_t)
#undef CA_SP_VT
}

template <typename YT>
void launch_prep(ca_engine* h, const double* logL, const double* extra) {
  hipLaunchKernelGGL((k_prep_cells<YT>), dim3((unsigned)h->N), dim3(CA_TB), 0, h->stream, (const YT*)h->Y, logL, extra, h->A, h->cn,
                     h->s64, h->s32, h->N, h->G, h->Gp, h->C, h->ovf_rowptr, h->ovf_col, h->ovf_val);
}

template <>
void launch_prep<uint8_t>(ca_engine* h, const double* logL, const double* extra) {
  if (!variant_on(h, CA_VAR_PREP_FAST, "CA_PREP_FAST")) {
    hipLaunchKernelGGL((k_prep_cells<uint8_t>), dim3((unsigned)h->N), dim3(CA_TB), 0, h->stream, (const uint8_t*)h->Y, logL, extra, h->A,
                       h->cn, h->s64, h->s32, h->N, h->G, h->Gp, h->C, h->ovf_rowptr, h->ovf_col, h->ovf_val);
    return;
  }
  const int grid = (int)std::min<int64_t>(cdiv(h->N, CA_TB / 64), (int64_t)h->n_cu * 8);
  hipLaunchKernelGGL(k_prep_cells_u8, dim3(grid), dim3(CA_TB), 0, h->stream, (const uint8_t*)h->Y, logL, extra, h->A, h->cn, h->s64,
                     h->s32, h->N, h->G, h->Gp, h->C, h->ovf_rowptr, h->ovf_col, h->ovf_val);
}

