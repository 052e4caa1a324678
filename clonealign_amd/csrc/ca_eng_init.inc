// ca_eng_init.inc -- part of clonealign_hip.hip (textually included there, in this order; one translation unit): C ABI, once per fit on the resident matrix: PCA initialisation of psi (transformed count-matrix pass, Gram-Schmidt and Jacobi on the host, blocked subspace iteration), per-clone gene sums, the squared error of a fit (ca_fit_mse), log-expression sums per gene and cell group (ca_logexpr_sums).  (The calls that score the matrix under a fitted model: ca_eng_score.inc.)
extern "C++" {   // (templates: this part sits inside the C ABI's extern "C" block)
namespace {
// Transformed pass over Y with explicit factor buffers (PCA init): row products Y'.Vp -> YWp, column products Y'^T.Fp -> YTp
template <int TF>
int ypass_tf(ca_engine* h, const float* Fp, const float* Vp, int q, float* YWp, float* YTp, float* csum) {
  dim3 grid((unsigned)((int64_t)h->nrg * h->nseg));
  const ca_ypass_ops ops = {Fp, q, Vp, YWp, YTp, q};
  ca_ovf_args no_ovf;   // (the overflow list: the three launches below)
  memset(&no_ovf, 0, sizeof(no_ovf));
  for (int koff = 0; koff < q; koff += 4) {
    const int kk = std::min(4, q - koff);
    ypass<TF>(h, ops, koff, kk, grid, no_ovf);
    HIPCK(h, hipGetLastError());
  }
  if (h->n_ovf > 0) {
    hipLaunchKernelGGL(k_ovf_rows, dim3(cdiv(h->N, CA_TB)), dim3(CA_TB), 0, h->stream, h->ovf_rowptr, h->ovf_col, h->ovf_val, Vp, q,
                       YWp + (int64_t)h->nseg * h->N * q, h->N, q, TF);
    hipLaunchKernelGGL(k_ovf_chunks, dim3(cdiv(h->n_ovf_chunk, CA_TB / 64)), dim3(CA_TB), 0, h->stream, h->ovf_chunk_start, h->ovf_row2,
                       h->ovf_val2, Fp, q, csum, h->n_ovf_chunk, q, TF);
    hipLaunchKernelGGL(k_ovf_cols, dim3(cdiv(h->Gp, CA_TB)), dim3(CA_TB), 0, h->stream, h->ovf_col_chunk_ptr, csum,
                       YTp + (int64_t)h->nrg * h->Gp * q, h->Gp, h->G, q);
    HIPCK(h, hipGetLastError());
  }
  return CA_OK;
}

// modified Gram-Schmidt (twice) on the columns of Q [G][q] (row-major), double precision
void orthonormalize(std::vector<double>& Q, int G, int q) {
  for (int rep = 0; rep < 2; ++rep)
    for (int k = 0; k < q; ++k) {
      for (int j = 0; j < k; ++j) {
        double d = 0.0;
        for (int g = 0; g < G; ++g) d += Q[(size_t)g * q + k] * Q[(size_t)g * q + j];
        for (int g = 0; g < G; ++g) Q[(size_t)g * q + k] -= d * Q[(size_t)g * q + j];
      }
      double nn = 0.0;
      for (int g = 0; g < G; ++g) nn += Q[(size_t)g * q + k] * Q[(size_t)g * q + k];
      nn = std::sqrt(nn);
      if (nn < 1e-300) nn = 1.0;
      for (int g = 0; g < G; ++g) Q[(size_t)g * q + k] /= nn;
    }
}
// cyclic Jacobi eigen-decomposition of a symmetric q x q matrix; eigenvalues descending, eigenvectors in columns of W
void sym_eig(std::vector<double> T, int q, std::vector<double>& lam, std::vector<double>& W) {
  W.assign((size_t)q * q, 0.0);
  for (int i = 0; i < q; ++i) W[(size_t)i * q + i] = 1.0;
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0.0;
    for (int i = 0; i < q; ++i) for (int j = i + 1; j < q; ++j) off += T[(size_t)i * q + j] * T[(size_t)i * q + j];
    if (off < 1e-30) break;
    for (int p_ = 0; p_ < q; ++p_)
      for (int r = p_ + 1; r < q; ++r) {
        const double apr = T[(size_t)p_ * q + r];
        if (std::fabs(apr) < 1e-300) continue;
        const double th = (T[(size_t)r * q + r] - T[(size_t)p_ * q + p_]) / (2.0 * apr);
        const double t = (th >= 0 ? 1.0 : -1.0) / (std::fabs(th) + std::sqrt(th * th + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), sn = t * c;
        for (int k = 0; k < q; ++k) {
          const double a = T[(size_t)k * q + p_], b = T[(size_t)k * q + r];
          T[(size_t)k * q + p_] = c * a - sn * b; T[(size_t)k * q + r] = sn * a + c * b;
        }
        for (int k = 0; k < q; ++k) {
          const double a = T[(size_t)p_ * q + k], b = T[(size_t)r * q + k];
          T[(size_t)p_ * q + k] = c * a - sn * b; T[(size_t)r * q + k] = sn * a + c * b;
        }
        for (int k = 0; k < q; ++k) {
          const double a = W[(size_t)k * q + p_], b = W[(size_t)k * q + r];
          W[(size_t)k * q + p_] = c * a - sn * b; W[(size_t)k * q + r] = sn * a + c * b;
        }
      }
  }
  std::vector<int> idx(q);
  for (int i = 0; i < q; ++i) idx[i] = i;
  std::sort(idx.begin(), idx.end(), [&](int a, int b) { return T[(size_t)a * q + a] > T[(size_t)b * q + b]; });
  lam.resize(q);
  std::vector<double> W2((size_t)q * q);
  for (int j = 0; j < q; ++j) {
    lam[j] = T[(size_t)idx[j] * q + idx[j]];
    for (int k = 0; k < q; ++k) W2[(size_t)k * q + j] = W[(size_t)k * q + idx[j]];
  }
  W = W2;
}
}  // namespace
}  // extern "C++"

// host-side all-reduce of a small double vector through the engine's transport (device scratch round trip)
static int allreduce_host_vec(ca_engine* h, std::vector<double>& v, double* dev_scratch) {
  if (!is_sharded(h)) return CA_OK;
  HIPCK(h, hipMemcpyAsync(dev_scratch, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  CACK(allreduce(h, dev_scratch, (int64_t)v.size()));
  HIPCK(h, hipMemcpyAsync(v.data(), dev_scratch, v.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  SYNC(h);
  return CA_OK;
}

int ca_init_psi_pca(ca_handle h, const double* noise, int32_t n_iter, uint64_t seed, double* pcs_out) {
  if (!h) return CA_ERR_INVALID;
  CA_NOT_IN_RUN(h);
  if (h->K == 0) return CA_OK;
  HIPCK(h, hipSetDevice(h->device));
  CACK(wait_y(h, true));
  const int64_t N = h->N; const int G = h->G, Gp = h->Gp, K = h->K;
  const int q = std::min(std::min(K + 4, 12), G);
  if (n_iter <= 0) n_iter = 40;
  std::vector<float> vp((size_t)Gp * q, 0.f);   // (what rows_pass uploads: declared before the owner of the device memory, which waits for the stream)
  std::vector<double> c(q), B;
  ca_call_mem mem(h);
  float *Fp = mem.alloc<float>(N * q), *Vp = mem.alloc<float>((int64_t)Gp * q), *YWp = mem.alloc<float>((int64_t)(h->nseg + 1) * N * q);
  float *YTp = mem.alloc<float>((int64_t)(h->nrb + 1) * Gp * q), *csum = mem.alloc<float>((int64_t)std::max(h->n_ovf_chunk, 1) * q);
  double *ytd = mem.alloc<double>(std::max<int64_t>((int64_t)Gp * q, 2 * (int64_t)Gp + q * q + 4 * q + 8)), *cdev = mem.alloc<double>(q);
  if (mem.rc != CA_OK) return mem.rc;
  const int nrb_tot = h->nrg + (h->n_ovf > 0 ? 1 : 0), nseg_tot = h->nseg + (h->n_ovf > 0 ? 1 : 0);
  auto colsum_to_host = [&](int qq, std::vector<double>& out) -> int {
    hipLaunchKernelGGL(k_colsum, dim3(cdiv((int64_t)Gp * qq, 64)), dim3(1024), 0, h->stream, YTp, ytd, nrb_tot, (int64_t)Gp * qq, Gp * qq);
    out.resize((size_t)G * qq);
    HIPCK(h, hipMemcpyAsync(out.data(), ytd, (size_t)G * qq * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    SYNC(h);
    return CA_OK;
  };
  int rc = CA_OK;
  // ---- column means and standard deviations of x = log2(y + 1)
  std::vector<double> sx, sxx, ntot(1, (double)N);
  {
    // float64 sums of x and x^2 per gene over the resident matrix (k_col_logstats), slices summed in order on the host; entries held
    // as 255 + overflow excess are put right from the host copy of the list (x = log2(256 + excess) where the dense byte gave 8)
    const int nsl = (int)std::max<int64_t>(1, std::min<int64_t>(128, N / 256));
    const int64_t rows_per = (N + nsl - 1) / nsl;
    ca_call_mem slices(h);
    double* part = slices.alloc<double>((int64_t)nsl * 2 * G);
    if (slices.rc != CA_OK) return slices.rc;
    const dim3 grid(cdiv(G, CA_TB), nsl);
    if (h->ystore == CA_YSTORE_U8) hipLaunchKernelGGL((k_col_logstats<uint8_t>), grid, dim3(CA_TB), 0, h->stream, (const uint8_t*)h->Y, N, G, Gp, rows_per, part);
    else if (h->ystore == CA_YSTORE_U16) hipLaunchKernelGGL((k_col_logstats<uint16_t>), grid, dim3(CA_TB), 0, h->stream, (const uint16_t*)h->Y, N, G, Gp, rows_per, part);
    else hipLaunchKernelGGL((k_col_logstats<float>), grid, dim3(CA_TB), 0, h->stream, (const float*)h->Y, N, G, Gp, rows_per, part);
    std::vector<double> hp((size_t)nsl * 2 * G);
    HIPCK(h, hipGetLastError());
    HIPCK(h, hipMemcpyAsync(hp.data(), part, hp.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));
    sx.assign((size_t)G, 0.0); sxx.assign((size_t)G, 0.0);
    for (int sl = 0; sl < nsl; ++sl)
      for (int g = 0; g < G; ++g) { sx[g] += hp[((size_t)sl * 2 + 0) * G + g]; sxx[g] += hp[((size_t)sl * 2 + 1) * G + g]; }
    for (int64_t i = 0; i < h->n_ovf; ++i) {
      const double x = std::log2(256.0 + (double)h->h_oval[(size_t)i]);
      sx[h->h_ocol[(size_t)i]] += x - 8.0; sxx[h->h_ocol[(size_t)i]] += x * x - 64.0;
    }
    std::vector<double> pack((size_t)2 * G + 1);
    for (int g = 0; g < G; ++g) { pack[g] = sx[g]; pack[G + g] = sxx[g]; }
    pack[2 * G] = (double)N;
    if ((rc = allreduce_host_vec(h, pack, ytd)) != CA_OK) return rc;
    for (int g = 0; g < G; ++g) { sx[g] = pack[g]; sxx[g] = pack[G + g]; }
    ntot[0] = pack[2 * G];
  }
  const double Nt = ntot[0];
  std::vector<double> mean(G), sd(G);
  for (int g = 0; g < G; ++g) {
    mean[g] = sx[g] / Nt;
    const double var = (sxx[g] - Nt * mean[g] * mean[g]) / (Nt - 1.0);
    sd[g] = std::sqrt(var);
    if (!(var > 1e-12 * std::max(1.0, mean[g] * mean[g]))) {
      h->err = "cannot rescale a constant/zero column to unit variance";   // prcomp(scale. = TRUE) on a constant gene
      return CA_ERR_INVALID;
    }
  }
  // ---- blocked subspace iteration on Xs^T Xs
  std::vector<double> Q((size_t)G * q);
  {
    std::vector<float> r((size_t)G * q);
    ca_philox::normal_draw(seed ^ 0x9E3779B97F4A7C15ull, 0, (int64_t)G * q, r.data());
    for (size_t i = 0; i < Q.size(); ++i) Q[i] = r[i];
    orthonormalize(Q, G, q);
  }
  auto rows_pass = [&]() -> int {   // A = Xs Q  ->  Fp
    for (int k = 0; k < q; ++k) c[k] = 0.0;
    for (int g = 0; g < G; ++g)
      for (int k = 0; k < q; ++k) {
        const double w = Q[(size_t)g * q + k] / sd[g];
        vp[(size_t)g * q + k] = (float)w;
        c[k] += mean[g] * w;
      }
    HIPCK(h, hipMemcpyAsync(Vp, vp.data(), vp.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIPCK(h, hipMemcpyAsync(cdev, c.data(), q * sizeof(double), hipMemcpyHostToDevice, h->stream));
    CACK(ypass_tf<1>(h, Fp, Vp, q, YWp, YTp, csum));
    hipLaunchKernelGGL(k_pca_rows, dim3(cdiv(N * q, CA_TB)), dim3(CA_TB), 0, h->stream, YWp, cdev, Fp, N, q, nseg_tot);
    HIPCK(h, hipGetLastError());
    return CA_OK;
  };
  for (int it = 0; it < n_iter && rc == CA_OK; ++it) {
    if ((rc = rows_pass()) != CA_OK) break;
    if ((rc = ypass_tf<1>(h, Fp, Vp, q, YWp, YTp, csum)) != CA_OK) break;   // B = Xs^T A (column products)
    if ((rc = colsum_to_host(q, B)) != CA_OK) break;
    if ((rc = allreduce_host_vec(h, B, ytd)) != CA_OK) break;
    for (int g = 0; g < G; ++g)
      for (int k = 0; k < q; ++k) Q[(size_t)g * q + k] = B[(size_t)g * q + k] / sd[g];
    orthonormalize(Q, G, q);
  }
  if (rc != CA_OK) return rc;
  // ---- Rayleigh-Ritz on the converged subspace
  if ((rc = rows_pass()) != CA_OK) return rc;
  std::vector<float> Af((size_t)N * q);
  HIPCK(h, hipMemcpyAsync(Af.data(), Fp, Af.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIPCK(h, hipStreamSynchronize(h->stream));
  std::vector<double> T((size_t)q * q, 0.0);
  for (int64_t n = 0; n < N; ++n)
    for (int a = 0; a < q; ++a)
      for (int b = a; b < q; ++b) T[(size_t)a * q + b] += (double)Af[(size_t)n * q + a] * (double)Af[(size_t)n * q + b];
  for (int a = 0; a < q; ++a) for (int b = 0; b < a; ++b) T[(size_t)a * q + b] = T[(size_t)b * q + a];
  if ((rc = allreduce_host_vec(h, T, ytd)) != CA_OK) return rc;
  std::vector<double> lam, W;
  sym_eig(T, q, lam, W);
  std::vector<double> sgn(K, 1.0);
  for (int k = 0; k < K; ++k) {   // sign: loading of largest magnitude positive
    double best = 0.0, val = 1.0;
    for (int g = 0; g < G; ++g) {
      double vgk = 0.0;
      for (int j = 0; j < q; ++j) vgk += Q[(size_t)g * q + j] * W[(size_t)j * q + k];
      if (std::fabs(vgk) > best) { best = std::fabs(vgk); val = vgk; }
    }
    sgn[k] = val < 0 ? -1.0 : 1.0;
  }
  std::vector<double> sc((size_t)N * K), stat((size_t)2 * K, 0.0);
  for (int64_t n = 0; n < N; ++n)
    for (int k = 0; k < K; ++k) {
      double v = 0.0;
      for (int j = 0; j < q; ++j) v += (double)Af[(size_t)n * q + j] * W[(size_t)j * q + k];
      v *= sgn[k];
      sc[(size_t)n * K + k] = v;
      stat[k] += v; stat[K + k] += v * v;
    }
  if ((rc = allreduce_host_vec(h, stat, ytd)) != CA_OK) return rc;
  std::vector<float> Fh;
  if ((rc = download_f(h, Fh, h->F, N * std::max(h->D, 1))) != CA_OK) return rc;
  for (int k = 0; k < K; ++k) {
    const double mu_ = stat[k] / Nt, sdk = std::sqrt((stat[K + k] - Nt * mu_ * mu_) / (Nt - 1.0));   // scale(pcs)
    for (int64_t n = 0; n < N; ++n) {
      double v = (sc[(size_t)n * K + k] - mu_) / sdk;
      if (noise) v += noise[hidx(h->layout, n, k, N, K)];
      if (pcs_out) pcs_out[hidx(h->layout, n, k, N, K)] = v;
      Fh[(size_t)n * h->D + k] = (float)v;
    }
  }
  CACK(upload_f(h, h->F, Fh));
  CACK(refresh_derived(h));
  SYNC(h);
  return CA_OK;
}

int ca_clone_gene_sums(ca_handle h, const int32_t* clone_of_cell, double* Tout, double* Syy) {
  if (!h || !clone_of_cell || !Tout || !Syy) return CA_ERR_INVALID;
  CA_NOT_IN_RUN(h);
  HIPCK(h, hipSetDevice(h->device));
  CACK(wait_y(h, true));
  const int64_t N = h->N; const int G = h->G, Gp = h->Gp, C = h->C;
  // the assigned cells, sorted by clone (stable: cells ascending within a clone)
  std::vector<int64_t> start((size_t)C + 1, 0);
  for (int64_t n = 0; n < N; ++n) {
    const int c = clone_of_cell[n];
    if (c >= C) { h->err = "clone index out of range"; return CA_ERR_INVALID; }
    if (c >= 0) start[(size_t)c + 1]++;
  }
  for (int c = 0; c < C; ++c) start[(size_t)c + 1] += start[(size_t)c];
  const int64_t M = start[(size_t)C];
  // pack = [T G x C | Syy G], summed in FLOAT64 from the resident counts: a float32 partial is exact only below 2^24, which 512 cells of a strip
  // block pass with u16 counts, one f32 count can, and a gene's overflow entries do -- and n Syy - Sy^2 of the correlation cancels the digits
  // a float32-accurate Syy has left.  Integer counts: every partial here is an integer, exact below 2^53.
  std::vector<double> pack((size_t)G * C + G, 0.0);
  ca_call_mem mem(h);
  if (M > 0) {
    std::vector<int64_t> rows((size_t)M), piece;
    std::vector<int> piece_clone;
    {
      std::vector<int64_t> fill(start.begin(), start.end() - 1);
      for (int64_t n = 0; n < N; ++n) { const int c = clone_of_cell[n]; if (c >= 0) rows[(size_t)fill[(size_t)c]++] = n; }
    }
    // pieces of the list for the blocks: at most 128 over all cells and at least 256 cells each (as the column statistics of the PCA are cut), cut at the clones
    const int64_t per = std::max<int64_t>(256, cdiv(M, (int64_t)128));
    for (int c = 0; c < C; ++c)
      for (int64_t r = start[(size_t)c]; r < start[(size_t)c + 1]; r += per) { piece.push_back(r); piece_clone.push_back(c); }
    const int np = (int)piece.size();
    piece.push_back(M);
    const int64_t* rows_d = mem.upload(rows);
    const int64_t* piece_d = mem.upload(piece);
    double* part = mem.alloc<double>((int64_t)np * 2 * G);
    if (mem.rc != CA_OK) return mem.rc;
    const dim3 grid(cdiv(G, CA_TB), np);
    if (h->ystore == CA_YSTORE_U8) hipLaunchKernelGGL((k_col_listsums<uint8_t>), grid, dim3(CA_TB), 0, h->stream, (const uint8_t*)h->Y, rows_d, piece_d, G, Gp, part);
    else if (h->ystore == CA_YSTORE_U16) hipLaunchKernelGGL((k_col_listsums<uint16_t>), grid, dim3(CA_TB), 0, h->stream, (const uint16_t*)h->Y, rows_d, piece_d, G, Gp, part);
    else hipLaunchKernelGGL((k_col_listsums<float>), grid, dim3(CA_TB), 0, h->stream, (const float*)h->Y, rows_d, piece_d, G, Gp, part);
    HIPCK(h, hipGetLastError());
    std::vector<double> hp((size_t)np * 2 * G);
    HIPCK(h, hipMemcpyAsync(hp.data(), part, hp.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));   // (the host vectors above are read by the copies until here)
    for (int p = 0; p < np; ++p)   // pieces in list order
      for (int g = 0; g < G; ++g) {
        pack[(size_t)g * C + piece_clone[(size_t)p]] += hp[((size_t)p * 2 + 0) * G + g];
        pack[(size_t)G * C + g] += hp[((size_t)p * 2 + 1) * G + g];
      }
    // entries held as 255 + overflow excess: put right in double from the host copy of the list, fixed (cell, gene) order
    for (int64_t e = 0; e < h->n_ovf; ++e) {
      const int c = clone_of_cell[h->h_orow[(size_t)e]];
      if (c < 0) continue;
      const double x = (double)h->h_oval[(size_t)e];
      pack[(size_t)h->h_ocol[(size_t)e] * C + c] += x;
      pack[(size_t)G * C + h->h_ocol[(size_t)e]] += (255.0 + x) * (255.0 + x) - 255.0 * 255.0;
    }
  }
  if (is_sharded(h)) {   // sharded: totals over all cells
    double* scratch = mem.alloc<double>((int64_t)pack.size());
    if (mem.rc != CA_OK) return mem.rc;
    CACK(allreduce_host_vec(h, pack, scratch));
  }
  for (int g = 0; g < G; ++g) { for (int c = 0; c < C; ++c) Tout[hidx(h->layout, g, c, G, C)] = pack[(size_t)g * C + c]; Syy[g] = pack[(size_t)G * C + g]; }
  return CA_OK;
}


// sum of v[lo, hi) by halves: a fixed order whose error grows with log2 of the length
static double pairwise_sum(const double* v, int64_t lo, int64_t hi) {
  if (hi - lo <= 8) { double s = 0.0; for (int64_t i = lo; i < hi; ++i) s += v[i]; return s; }
  const int64_t mid = lo + (hi - lo) / 2;
  return pairwise_sum(v, lo, mid) + pairwise_sum(v, mid, hi);
}

// compute_ca_fit_mse (R/clonealign.R:415-434) on the resident matrix.  Reads the matrix, the row sums and the overflow list only: no wait for the loop's side
// stream, no variable, Adam slot or draw index changes.  A sharded handle takes part in the collective even when ITS input is invalid (the flag travels
// with the sums), so that every rank returns the same code instead of one of them leaving the others waiting.
int ca_fit_mse(ca_handle h, const int32_t* clone_of_cell, const double* E, double* sse_total, int64_t* n_cells_used, double* sse_gene, double* sse_cell) {
  if (!h || !clone_of_cell || !E || !sse_total || !n_cells_used) return CA_ERR_INVALID;
  CA_NOT_IN_RUN(h);
  HIPCK(h, hipSetDevice(h->device));
  const int64_t N = h->N; const int G = h->G, Gp = h->Gp, C = h->C, nseg = h->nseg;
  std::string bad;
  // the table: finite, clone-major and zero padded for the device, its column sums in gene order
  std::vector<double> Et((size_t)C * Gp, 0.0), esum((size_t)C, 0.0);
  for (int c = 0; c < C && bad.empty(); ++c)
    for (int g = 0; g < G; ++g) {
      const double v = E[hidx(h->layout, g, c, G, C)];
      if (!std::isfinite(v)) { bad = "predicted expression has a non-finite entry (gene " + std::to_string(g) + ", clone " + std::to_string(c) + ")"; break; }
      Et[(size_t)c * Gp + g] = v;
      esum[(size_t)c] += v;
    }
  // the used cells, sorted by clone (stable: cells ascending within a clone)
  std::vector<int64_t> start((size_t)C + 1, 0);
  for (int64_t n = 0; n < N && bad.empty(); ++n) {
    const int c = clone_of_cell[n];
    if (c < -1 || c >= C) bad = "clone index " + std::to_string(c) + " of cell " + std::to_string(n) + " is outside [-1, " + std::to_string(C) + ")";
    else if (c >= 0) start[(size_t)c + 1]++;
  }
  for (int c = 0; c < C && bad.empty(); ++c)
    if (start[(size_t)c + 1] > 0 && (!std::isfinite(esum[(size_t)c]) || esum[(size_t)c] == 0.0))
      bad = "predicted expression of clone " + std::to_string(c) + ", which is in use, sums to " + std::to_string(esum[(size_t)c]) + " over the genes";
  if (!bad.empty() && !is_sharded(h)) { h->err = "ca_fit_mse: " + bad; return CA_ERR_INVALID; }
  for (int c = 0; c < C; ++c) start[(size_t)c + 1] += start[(size_t)c];
  const int64_t M = bad.empty() ? start[(size_t)C] : 0;
  std::vector<double> gene((size_t)Gp, 0.0), cell;
  if (M > 0) {
    std::vector<int2> list((size_t)M);
    {
      std::vector<int64_t> fill(start.begin(), start.end() - 1);
      for (int64_t n = 0; n < N; ++n) { const int c = clone_of_cell[n]; if (c >= 0) list[(size_t)fill[(size_t)c]++] = make_int2((int)n, c); }
    }
    // strips of TR list entries per wave: as long as the grid still holds four blocks per CU (short strips mean more rows of genepart to add up)
    int TR = 256;
    while (TR > 32 && (int64_t)nseg * cdiv(cdiv(M, TR), CA_TB / 64) < 4 * (int64_t)h->n_cu) TR /= 2;
    ca_mse_ops o;
    o.M = M; o.TR = TR; o.nrb = cdiv(M, TR); o.nrg = cdiv(o.nrb, CA_TB / 64);
    ca_call_mem mem(h);
    const int2* list_d = mem.upload(list);
    const double *Et_d = mem.upload(Et), *esum_d = mem.upload(esum);
    ca_mse_row* meta = mem.alloc<ca_mse_row>(M);
    double *cellpart = mem.alloc<double>((int64_t)nseg * M), *genepart = mem.alloc<double>((int64_t)o.nrg * Gp), *gene_d = mem.alloc<double>(Gp), *cell_d = mem.alloc<double>(N);
    if (mem.rc != CA_OK) return mem.rc;
    HIPCK(h, hipMemsetAsync(cell_d, 0, (size_t)N * sizeof(double), h->stream));
    hipLaunchKernelGGL(k_mse_prep, dim3(cdiv(M, CA_TB)), dim3(CA_TB), 0, h->stream, list_d, h->s64, esum_d, h->n_ovf > 0 ? h->ovf_rowptr : nullptr, meta, M);
    HIPCK(h, hipGetLastError());
    o.meta = meta; o.Et = Et_d; o.cellpart = cellpart; o.genepart = genepart;
    CACK(launch_fit_mse(h, o));
    const int nb_gene = cdiv(Gp, 64);
    hipLaunchKernelGGL(k_mse_finish, dim3(nb_gene + cdiv(M, 1024)), dim3(1024), 0, h->stream, genepart, o.nrg, Gp, gene_d, cellpart, meta, M, (int)nseg, cell_d, nb_gene);
    HIPCK(h, hipGetLastError());
    HIPCK(h, hipMemcpyAsync(gene.data(), gene_d, (size_t)Gp * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (sse_cell) {
      cell.resize((size_t)N);
      HIPCK(h, hipMemcpyAsync(cell.data(), cell_d, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    HIPCK(h, hipStreamSynchronize(h->stream));   // (the host vectors above are read by the copies until here)
  }
  double n_used = (double)M;
  if (is_sharded(h)) {   // totals over all ranks: [sse_gene G | cells used | ranks whose input was refused]
    std::vector<double> pack(gene.begin(), gene.begin() + G);
    pack.push_back(n_used); pack.push_back(bad.empty() ? 0.0 : 1.0);
    ca_call_mem mem(h);
    double* scratch = mem.alloc<double>((int64_t)pack.size());
    if (mem.rc != CA_OK) return mem.rc;
    CACK(allreduce_host_vec(h, pack, scratch));
    if (pack[(size_t)G + 1] != 0.0) { h->err = "ca_fit_mse: " + (bad.empty() ? std::string("another rank refused its input") : bad); return CA_ERR_INVALID; }
    std::copy(pack.begin(), pack.begin() + G, gene.begin());
    n_used = pack[(size_t)G];
  }
  *sse_total = pairwise_sum(gene.data(), 0, G);
  *n_cells_used = (int64_t)n_used;
  if (sse_gene) std::copy(gene.begin(), gene.begin() + G, sse_gene);
  if (sse_cell) { if (M > 0) std::copy(cell.begin(), cell.end(), sse_cell); else std::fill(sse_cell, sse_cell + N, 0.0); }
  return CA_OK;
}

// The data side of plot_clonealign (R/plotting.R:177-205) on the resident matrix: S1[g][q] = sum over the cells of group q of lc_ng, S2[g] = sum over all used
// cells of lc_ng^2, lc_ng = log2(y_ng / sf_n + 1).  Like ca_fit_mse it reads the matrix, the row sums and the overflow list only: no wait for the loop's side
// stream, no variable, Adam slot or draw index changes.  A sharded handle takes part in both collectives (the used cells' library sizes for the default size
// factors, then the sums) even when ITS input is refused: the verdict travels with the numbers, so that every rank returns the same code.
int ca_logexpr_sums(ca_handle h, const int32_t* group_of_cell, int32_t n_groups, const double* size_factor, double* S1, double* S2, int64_t* n_group) {
  if (!h || !group_of_cell || !S1 || !S2 || !n_group) return CA_ERR_INVALID;
  CA_NOT_IN_RUN(h);
  if (n_groups < 1 || n_groups > 64) { h->err = "ca_logexpr_sums: n_groups = " + std::to_string(n_groups) + " is outside [1, 64]"; return CA_ERR_INVALID; }   // (the same on every rank: no collective)
  HIPCK(h, hipSetDevice(h->device));
  const int64_t N = h->N; const int G = h->G, Gp = h->Gp, Q = n_groups, nseg = h->nseg;
  std::string bad;
  // the used cells, sorted by group (stable: cells ascending within a group)
  std::vector<int64_t> start((size_t)Q + 1, 0);
  for (int64_t n = 0; n < N && bad.empty(); ++n) {
    const int q = group_of_cell[n];
    if (q < -1 || q >= Q) bad = "group index " + std::to_string(q) + " of cell " + std::to_string(n) + " is outside [-1, " + std::to_string(Q) + ")";
    else if (q >= 0) start[(size_t)q + 1]++;
  }
  if (!bad.empty()) std::fill(start.begin(), start.end(), 0);
  for (int q = 0; q < Q; ++q) start[(size_t)q + 1] += start[(size_t)q];
  int64_t M = start[(size_t)Q];
  std::vector<int2> list((size_t)M);
  {
    std::vector<int64_t> fill(start.begin(), start.end() - 1);
    for (int64_t n = 0; n < N && M > 0; ++n) { const int q = group_of_cell[n]; if (q >= 0) list[(size_t)fill[(size_t)q]++] = make_int2((int)n, q); }
  }
  // size factors in list order: the caller's, or library sizes over their mean over the used cells of ALL ranks (scater's library-size factors, centred at 1)
  std::vector<double> sf((size_t)M);
  double lib_sum = 0.0;
  if (size_factor) {
    for (int64_t i = 0; i < M; ++i) sf[(size_t)i] = size_factor[list[(size_t)i].x];
  } else {
    std::vector<double> rs((size_t)N), lib;
    HIPCK(h, hipMemcpyAsync(rs.data(), h->s64, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    SYNC(h);
    for (int64_t i = 0; i < M; ++i) sf[(size_t)i] = rs[(size_t)list[(size_t)i].x];
    lib.reserve((size_t)M);   // in cell order, so that the sum does not depend on the grouping
    for (int64_t n = 0; n < N && M > 0; ++n) if (group_of_cell[n] >= 0) lib.push_back(rs[(size_t)n]);
    lib_sum = pairwise_sum(lib.data(), 0, (int64_t)lib.size());
  }
  {
    std::vector<double> pack{lib_sum, (double)M, bad.empty() ? 0.0 : 1.0};   // [the used cells' library sizes | used cells | ranks whose input was refused]
    if (is_sharded(h)) {
      ca_call_mem mem(h);
      double* scratch = mem.alloc<double>((int64_t)pack.size());
      if (mem.rc != CA_OK) return mem.rc;
      CACK(allreduce_host_vec(h, pack, scratch));
    }
    if (pack[2] != 0.0) { h->err = "ca_logexpr_sums: " + (bad.empty() ? std::string("another rank refused its input") : bad); return CA_ERR_INVALID; }
    if (!size_factor && pack[1] > 0.0) {
      const double mean = pack[0] / pack[1];
      for (int64_t i = 0; i < M; ++i) sf[(size_t)i] = mean > 0.0 ? sf[(size_t)i] / mean : 0.0;
    }
  }
  for (int64_t i = 0; i < M; ++i)
    if (!(sf[(size_t)i] > 0.0) || !std::isfinite(sf[(size_t)i])) {
      bad = "cell " + std::to_string(list[(size_t)i].x) + " (group " + std::to_string(list[(size_t)i].y) + ") has size factor " + std::to_string(sf[(size_t)i]) +
            (size_factor ? "" : " (library size over the mean library size)") + ": it must be positive and finite";
      break;
    }
  if (!bad.empty() && !is_sharded(h)) { h->err = "ca_logexpr_sums: " + bad; return CA_ERR_INVALID; }
  if (!bad.empty()) M = 0;
  std::vector<double> sums((size_t)(Q + 1) * Gp, 0.0);   // [S1 of group 0 .. Q-1 | S2], each Gp values
  if (M > 0) {
    for (int64_t i = 0; i < M; ++i) sf[(size_t)i] = 1.0 / sf[(size_t)i];
    // block pieces of at most 4 TR list entries, cut at the group boundaries; TR as long as the grid still holds four blocks per CU
    auto pieces = [&](int tr) { int64_t p = 0; for (int q = 0; q < Q; ++q) p += cdiv(start[(size_t)q + 1] - start[(size_t)q], (int64_t)(CA_TB / 64) * tr); return p; };
    int TR = 256;
    while (TR > 32 && (int64_t)nseg * pieces(TR) < 4 * (int64_t)h->n_cu) TR /= 2;
    const int64_t BR = (int64_t)(CA_TB / 64) * TR;
    std::vector<ca_lx_blk> blk;
    std::vector<int> first((size_t)Q + 1, 0);
    for (int q = 0; q < Q; ++q) {
      for (int64_t r = start[(size_t)q]; r < start[(size_t)q + 1]; r += BR) {
        ca_lx_blk b; b.r0 = r; b.nrows = (int)std::min<int64_t>(BR, start[(size_t)q + 1] - r); b.pad = 0;
        blk.push_back(b);
      }
      first[(size_t)q + 1] = (int)blk.size();
    }
    ca_lx_ops o;
    o.nrg = (int)blk.size();
    ca_call_mem mem(h);
    const int2* list_d = mem.upload(list);
    const double* inv_d = mem.upload(sf);
    const ca_lx_blk* blk_d = mem.upload(blk);
    const int* first_d = mem.upload(first);
    ca_mse_row* meta = mem.alloc<ca_mse_row>(M);
    double *part1 = mem.alloc<double>((int64_t)o.nrg * Gp), *part2 = mem.alloc<double>((int64_t)o.nrg * Gp), *sums_d = mem.alloc<double>((int64_t)sums.size());
    if (mem.rc != CA_OK) return mem.rc;
    hipLaunchKernelGGL(k_lx_prep, dim3(cdiv(M, CA_TB)), dim3(CA_TB), 0, h->stream, list_d, inv_d, h->n_ovf > 0 ? h->ovf_rowptr : nullptr, meta, M);
    HIPCK(h, hipGetLastError());
    o.meta = meta; o.blk = blk_d; o.part1 = part1; o.part2 = part2;
    CACK(launch_logexpr(h, o));
    hipLaunchKernelGGL(k_lx_finish, dim3(cdiv(Gp, 64), Q + 1), dim3(1024), 0, h->stream, part1, part2, first_d, Q, Gp, sums_d);
    HIPCK(h, hipGetLastError());
    HIPCK(h, hipMemcpyAsync(sums.data(), sums_d, sums.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));   // (the host vectors above are read by the copies until here)
  }
  std::vector<double> cnt((size_t)Q, 0.0);
  if (bad.empty()) for (int q = 0; q < Q; ++q) cnt[(size_t)q] = (double)(start[(size_t)q + 1] - start[(size_t)q]);
  if (is_sharded(h)) {   // totals over all ranks: [S1 Q x G | S2 G | cells per group Q | ranks whose input was refused]
    std::vector<double> pack;
    pack.reserve((size_t)(Q + 1) * G + Q + 1);
    for (int q = 0; q <= Q; ++q) pack.insert(pack.end(), sums.begin() + (size_t)q * Gp, sums.begin() + (size_t)q * Gp + G);
    pack.insert(pack.end(), cnt.begin(), cnt.end());
    pack.push_back(bad.empty() ? 0.0 : 1.0);
    ca_call_mem mem(h);
    double* scratch = mem.alloc<double>((int64_t)pack.size());
    if (mem.rc != CA_OK) return mem.rc;
    CACK(allreduce_host_vec(h, pack, scratch));
    if (pack.back() != 0.0) { h->err = "ca_logexpr_sums: " + (bad.empty() ? std::string("another rank refused its input") : bad); return CA_ERR_INVALID; }
    for (int q = 0; q <= Q; ++q) std::copy(pack.begin() + (size_t)q * G, pack.begin() + (size_t)(q + 1) * G, sums.begin() + (size_t)q * Gp);
    std::copy(pack.begin() + (size_t)(Q + 1) * G, pack.begin() + (size_t)(Q + 1) * G + Q, cnt.begin());
  }
  for (int g = 0; g < G; ++g) {
    for (int q = 0; q < Q; ++q) S1[hidx(h->layout, g, q, G, Q)] = sums[(size_t)q * Gp + g];
    S2[g] = sums[(size_t)Q * Gp + g];
  }
  for (int q = 0; q < Q; ++q) n_group[q] = (int64_t)cnt[(size_t)q];
  return CA_OK;
}
