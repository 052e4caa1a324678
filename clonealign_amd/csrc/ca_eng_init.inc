// ca_eng_init.inc -- part of clonealign_hip.hip (textually included there, in this order; one translation unit): C ABI, once per fit on the resident matrix: PCA initialisation of psi (transformed count-matrix pass, Gram-Schmidt and Jacobi on the host, blocked subspace iteration), per-clone gene sums, the squared error of a fit (ca_fit_mse), the per-cell, per-clone log-likelihood under a fit (ca_clone_loglik), the per-cell MAP psi of cells outside a fit (ca_project_cells), log-expression sums per gene and cell group (ca_logexpr_sums).
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
  float *Fp = nullptr, *Vp = nullptr, *YWp = nullptr, *YTp = nullptr, *csum = nullptr; double *ytd = nullptr, *cdev = nullptr;
  auto cleanup = [&]() { hipFree(Fp); hipFree(Vp); hipFree(YWp); hipFree(YTp); hipFree(csum); hipFree(ytd); hipFree(cdev); };
#define PCK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { h->err = std::string(#call) + ": " + hipGetErrorString(e_); cleanup(); return CA_ERR_HIP; } } while (0)
  PCK(hipMalloc((void**)&Fp, (size_t)N * q * sizeof(float)));
  PCK(hipMalloc((void**)&Vp, (size_t)Gp * q * sizeof(float)));
  PCK(hipMalloc((void**)&YWp, (size_t)(h->nseg + 1) * N * q * sizeof(float)));
  PCK(hipMalloc((void**)&YTp, (size_t)(h->nrb + 1) * Gp * q * sizeof(float)));
  PCK(hipMalloc((void**)&csum, (size_t)std::max(h->n_ovf_chunk, 1) * q * sizeof(float)));
  PCK(hipMalloc((void**)&ytd, (size_t)std::max<int64_t>((int64_t)Gp * q, 2 * (int64_t)Gp + q * q + 4 * q + 8) * sizeof(double)));
  PCK(hipMalloc((void**)&cdev, (size_t)q * sizeof(double)));
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
    double* part = nullptr;
    PCK(hipMalloc((void**)&part, (size_t)nsl * 2 * G * sizeof(double)));
    const dim3 grid(cdiv(G, CA_TB), nsl);
    if (h->ystore == CA_YSTORE_U8) hipLaunchKernelGGL((k_col_logstats<uint8_t>), grid, dim3(CA_TB), 0, h->stream, (const uint8_t*)h->Y, N, G, Gp, rows_per, part);
    else if (h->ystore == CA_YSTORE_U16) hipLaunchKernelGGL((k_col_logstats<uint16_t>), grid, dim3(CA_TB), 0, h->stream, (const uint16_t*)h->Y, N, G, Gp, rows_per, part);
    else hipLaunchKernelGGL((k_col_logstats<float>), grid, dim3(CA_TB), 0, h->stream, (const float*)h->Y, N, G, Gp, rows_per, part);
    std::vector<double> hp((size_t)nsl * 2 * G);
    hipError_t e1 = hipGetLastError();
    if (e1 == hipSuccess) e1 = hipMemcpyAsync(hp.data(), part, hp.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    if (e1 == hipSuccess) e1 = hipStreamSynchronize(h->stream);
    hipFree(part);
    PCK(e1);
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
    if ((rc = allreduce_host_vec(h, pack, ytd)) != CA_OK) { cleanup(); return rc; }
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
      cleanup();
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
  std::vector<float> vp((size_t)Gp * q, 0.f);
  std::vector<double> c(q), B;
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
  if (rc != CA_OK) { cleanup(); return rc; }
  // ---- Rayleigh-Ritz on the converged subspace
  if ((rc = rows_pass()) != CA_OK) { cleanup(); return rc; }
  std::vector<float> Af((size_t)N * q);
  PCK(hipMemcpyAsync(Af.data(), Fp, Af.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  PCK(hipStreamSynchronize(h->stream));
  std::vector<double> T((size_t)q * q, 0.0);
  for (int64_t n = 0; n < N; ++n)
    for (int a = 0; a < q; ++a)
      for (int b = a; b < q; ++b) T[(size_t)a * q + b] += (double)Af[(size_t)n * q + a] * (double)Af[(size_t)n * q + b];
  for (int a = 0; a < q; ++a) for (int b = 0; b < a; ++b) T[(size_t)a * q + b] = T[(size_t)b * q + a];
  if ((rc = allreduce_host_vec(h, T, ytd)) != CA_OK) { cleanup(); return rc; }
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
  if ((rc = allreduce_host_vec(h, stat, ytd)) != CA_OK) { cleanup(); return rc; }
  std::vector<float> Fh;
  if ((rc = download_f(h, Fh, h->F, N * std::max(h->D, 1))) != CA_OK) { cleanup(); return rc; }
  for (int k = 0; k < K; ++k) {
    const double mu_ = stat[k] / Nt, sdk = std::sqrt((stat[K + k] - Nt * mu_ * mu_) / (Nt - 1.0));   // scale(pcs)
    for (int64_t n = 0; n < N; ++n) {
      double v = (sc[(size_t)n * K + k] - mu_) / sdk;
      if (noise) v += noise[hidx(h->layout, n, k, N, K)];
      if (pcs_out) pcs_out[hidx(h->layout, n, k, N, K)] = v;
      Fh[(size_t)n * h->D + k] = (float)v;
    }
  }
  rc = upload_f(h, h->F, Fh);
  cleanup();
  if (rc != CA_OK) return rc;
  CACK(refresh_derived(h));
  SYNC(h);
  return CA_OK;
#undef PCK
}

int ca_clone_gene_sums(ca_handle h, const int32_t* clone_of_cell, double* Tout, double* Syy) {
  if (!h || !clone_of_cell || !Tout || !Syy) return CA_ERR_INVALID;
  CA_NOT_IN_RUN(h);
  HIPCK(h, hipSetDevice(h->device));
  CACK(wait_y(h, true));
  const int64_t N = h->N; const int G = h->G, Gp = h->Gp, C = h->C;
  float *Fp = nullptr, *Vp = nullptr, *YWp = nullptr, *YTp = nullptr, *csum = nullptr; double* ytd = nullptr;
  auto cleanup = [&]() { hipFree(Fp); hipFree(Vp); hipFree(YWp); hipFree(YTp); hipFree(csum); hipFree(ytd); };
#define PCK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { h->err = std::string(#call) + ": " + hipGetErrorString(e_); cleanup(); return CA_ERR_HIP; } } while (0)
  PCK(hipMalloc((void**)&Fp, (size_t)N * C * sizeof(float)));
  PCK(hipMalloc((void**)&Vp, (size_t)Gp * C * sizeof(float)));
  PCK(hipMalloc((void**)&YWp, (size_t)(h->nseg + 1) * N * C * sizeof(float)));
  PCK(hipMalloc((void**)&YTp, (size_t)(h->nrb + 1) * Gp * C * sizeof(float)));
  PCK(hipMalloc((void**)&csum, (size_t)std::max(h->n_ovf_chunk, 1) * C * sizeof(float)));
  PCK(hipMalloc((void**)&ytd, (size_t)Gp * C * sizeof(double)));
  PCK(hipMemsetAsync(Vp, 0, (size_t)Gp * C * sizeof(float), h->stream));
  const int nrb_tot = h->nrg + (h->n_ovf > 0 ? 1 : 0);
  std::vector<float> ind((size_t)N * C, 0.f), asg((size_t)N, 0.f);
  for (int64_t n = 0; n < N; ++n) {
    const int c = clone_of_cell[n];
    if (c >= C) { h->err = "clone index out of range"; cleanup(); return CA_ERR_INVALID; }
    if (c >= 0) { ind[(size_t)n * C + c] = 1.f; asg[n] = 1.f; }
  }
  int rc;
  std::vector<double> out;
  // T = Y^T I  (strip partials are exact integers below 2^24 for integer counts; the cross-strip sum is fp64)
  PCK(hipMemcpyAsync(Fp, ind.data(), ind.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
  if ((rc = ypass_tf<0>(h, Fp, Vp, C, YWp, YTp, csum)) != CA_OK) { cleanup(); return rc; }
  hipLaunchKernelGGL(k_colsum, dim3(cdiv((int64_t)Gp * C, 64)), dim3(1024), 0, h->stream, YTp, ytd, nrb_tot, (int64_t)Gp * C, Gp * C);
  out.resize((size_t)G * C);
  PCK(hipMemcpyAsync(out.data(), ytd, out.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  PCK(hipStreamSynchronize(h->stream));
  for (int g = 0; g < G; ++g)
    for (int c = 0; c < C; ++c) Tout[hidx(h->layout, g, c, G, C)] = out[(size_t)g * C + c];
  // Syy = (Y^2)^T 1_assigned
  PCK(hipMemcpyAsync(Fp, asg.data(), asg.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
  if ((rc = ypass_tf<3>(h, Fp, Vp, 1, YWp, YTp, csum)) != CA_OK) { cleanup(); return rc; }
  hipLaunchKernelGGL(k_colsum, dim3(cdiv((int64_t)Gp, 64)), dim3(1024), 0, h->stream, YTp, ytd, nrb_tot, (int64_t)Gp, Gp);
  PCK(hipMemcpyAsync(Syy, ytd, (size_t)G * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  PCK(hipStreamSynchronize(h->stream));
  cleanup();
  if (is_sharded(h)) {   // sharded: totals over all cells
    std::vector<double> pack((size_t)G * C + G);
    for (int g = 0; g < G; ++g) { for (int c = 0; c < C; ++c) pack[(size_t)g * C + c] = out[(size_t)g * C + c]; pack[(size_t)G * C + g] = Syy[g]; }
    double* scratch = nullptr;
    HIPCK(h, hipMalloc((void**)&scratch, pack.size() * sizeof(double)));
    rc = allreduce_host_vec(h, pack, scratch);
    hipFree(scratch);
    if (rc != CA_OK) return rc;
    for (int g = 0; g < G; ++g) { for (int c = 0; c < C; ++c) Tout[hidx(h->layout, g, c, G, C)] = pack[(size_t)g * C + c]; Syy[g] = pack[(size_t)G * C + g]; }
  }
  return CA_OK;
#undef PCK
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
  int2* list_d = nullptr; ca_mse_row* meta = nullptr; double *Et_d = nullptr, *esum_d = nullptr, *cellpart = nullptr, *genepart = nullptr, *gene_d = nullptr, *cell_d = nullptr;
  auto cleanup = [&]() { hipFree(list_d); hipFree(meta); hipFree(Et_d); hipFree(esum_d); hipFree(cellpart); hipFree(genepart); hipFree(gene_d); hipFree(cell_d); };
#define PCK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { h->err = std::string(#call) + ": " + hipGetErrorString(e_); cleanup(); return CA_ERR_HIP; } } while (0)
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
    PCK(hipMalloc((void**)&list_d, (size_t)M * sizeof(int2)));
    PCK(hipMalloc((void**)&meta, (size_t)M * sizeof(ca_mse_row)));
    PCK(hipMalloc((void**)&Et_d, Et.size() * sizeof(double)));
    PCK(hipMalloc((void**)&esum_d, (size_t)C * sizeof(double)));
    PCK(hipMalloc((void**)&cellpart, (size_t)nseg * M * sizeof(double)));
    PCK(hipMalloc((void**)&genepart, (size_t)o.nrg * Gp * sizeof(double)));
    PCK(hipMalloc((void**)&gene_d, (size_t)Gp * sizeof(double)));
    PCK(hipMalloc((void**)&cell_d, (size_t)N * sizeof(double)));
    PCK(hipMemcpyAsync(list_d, list.data(), (size_t)M * sizeof(int2), hipMemcpyHostToDevice, h->stream));
    PCK(hipMemcpyAsync(Et_d, Et.data(), Et.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    PCK(hipMemcpyAsync(esum_d, esum.data(), (size_t)C * sizeof(double), hipMemcpyHostToDevice, h->stream));
    PCK(hipMemsetAsync(cell_d, 0, (size_t)N * sizeof(double), h->stream));
    hipLaunchKernelGGL(k_mse_prep, dim3(cdiv(M, CA_TB)), dim3(CA_TB), 0, h->stream, list_d, h->s64, esum_d, h->n_ovf > 0 ? h->ovf_rowptr : nullptr, meta, M);
    PCK(hipGetLastError());
    o.meta = meta; o.Et = Et_d; o.cellpart = cellpart; o.genepart = genepart;
    { const int rc = launch_fit_mse(h, o); if (rc != CA_OK) { cleanup(); return rc; } }
    const int nb_gene = cdiv(Gp, 64);
    hipLaunchKernelGGL(k_mse_finish, dim3(nb_gene + cdiv(M, 1024)), dim3(1024), 0, h->stream, genepart, o.nrg, Gp, gene_d, cellpart, meta, M, (int)nseg, cell_d, nb_gene);
    PCK(hipGetLastError());
    PCK(hipMemcpyAsync(gene.data(), gene_d, (size_t)Gp * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (sse_cell) {
      cell.resize((size_t)N);
      PCK(hipMemcpyAsync(cell.data(), cell_d, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    PCK(hipStreamSynchronize(h->stream));   // (the host vectors above are read by the copies until here)
    cleanup();
  }
#undef PCK
  double n_used = (double)M;
  if (is_sharded(h)) {   // totals over all ranks: [sse_gene G | cells used | ranks whose input was refused]
    std::vector<double> pack(gene.begin(), gene.begin() + G);
    pack.push_back(n_used); pack.push_back(bad.empty() ? 0.0 : 1.0);
    double* scratch = nullptr;
    HIPCK(h, hipMalloc((void**)&scratch, pack.size() * sizeof(double)));
    const int rc = allreduce_host_vec(h, pack, scratch);
    hipFree(scratch);
    if (rc != CA_OK) return rc;
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

// The table of the log-likelihood sweep (k_clone_ll; ca_clone_loglik and ca_project_cells): per gene the columns [log E of the clones | V], in groups of NC
// columns, zero padded; where E = 0 the entry is 0 and the gene's mask has the bit.  logz0[c] = log sum_g E[g][c].  Returns the refusal, or "".
extern "C++" {
namespace {
std::string ll_sweep_table(ca_engine* h, const double* E, const double* V, int D, int NC, int ngrp, std::vector<double>& tab, std::vector<unsigned>& zmask, std::vector<double>& logz0) {
  const int G = h->G, Gp = h->Gp, C = h->C;
  std::string bad;
  std::vector<double> col((size_t)G);
  tab.assign((size_t)ngrp * Gp * NC, 0.0); logz0.assign((size_t)C, 0.0); zmask.assign((size_t)ngrp * Gp, 0u);
  for (int c = 0; c < C && bad.empty(); ++c) {
    const int grp = c / NC, cc = c % NC;
    for (int g = 0; g < G; ++g) {
      const double v = E[hidx(h->layout, g, c, G, C)];
      if (!std::isfinite(v) || v < 0.0) { bad = "expected expression has a negative or non-finite entry (gene " + std::to_string(g) + ", clone " + std::to_string(c) + ")"; break; }
      col[(size_t)g] = v;
      if (v > 0.0) tab[((size_t)grp * Gp + g) * NC + cc] = std::log(v);
      else zmask[(size_t)grp * Gp + g] |= 1u << cc;
    }
    if (!bad.empty()) break;
    const double sum = pairwise_sum(col.data(), 0, G);
    if (!std::isfinite(sum) || sum == 0.0) { bad = "expected expression of clone " + std::to_string(c) + " sums to " + std::to_string(sum) + " over the genes"; break; }
    logz0[(size_t)c] = std::log(sum);
  }
  for (int g = 0; g < G && D > 0 && bad.empty(); ++g)
    for (int d = 0; d < D; ++d) {
      const double v = V[hidx(h->layout, g, d, G, D)];
      if (!std::isfinite(v)) { bad = "V has a non-finite entry (gene " + std::to_string(g) + ", factor " + std::to_string(d) + ")"; break; }
      tab[((size_t)((C + d) / NC) * Gp + g) * NC + (C + d) % NC] = v;
    }
  return bad;
}
}  // namespace
}  // extern "C++"

// p_y_on_c (R/inference-tflow.R:288-296) at a fit's point estimates on the resident matrix: ll[n][c] for every cell and clone (include/clonealign_hip.h has the
// formula and the rules).  Like ca_fit_mse it reads the matrix, the row sums and the overflow list only: no wait for the loop's side stream, no variable, Adam
// slot or draw index changes.  U and ll cover the local cells, so a sharded handle needs no sums from its peers; it still takes part in ONE small collective,
// the verdict on the input (a non-finite U is local), so that every rank returns the same code instead of one of them leaving the others waiting.
// ONE body serves ca_clone_loglik and ca_clone_pair_loglik: the pair call runs the same launches over its cell range -- its ll is ca_clone_loglik's bit for bit,
// and the pair-independent pieces (sum y eta, the lgamma sum, log Z) are those launches' -- and then, per batch, k_pair_cell and k_pair_ll (D > 0) or the
// table sweep of k_clone_ll with k_pair_tab_finish (D = 0).  ca_clone_loglik_dm is a third caller: after the same launches, per batch, k_dm_cell and k_dm_ll (every D).
extern "C++" {
namespace {
struct ca_pair_req { const double* weights; int W; double* pair_ll; };   // the pair part of a call: W weights in (0, 1), the output cell_cnt x (M W)
struct ca_dm_req { const double* conc; int K; double* dm_ll; };          // the Dirichlet-multinomial part of a call: K concentrations > 0, the output cell_cnt x (C K)
int clone_ll_impl(ca_engine* h, const char* who, const double* E, const double* U, const double* V, int32_t D, int32_t with_const, int64_t c_lo, int64_t c_cnt, double* ll,
                  const ca_pair_req* pq, const ca_dm_req* dq = nullptr) {
  const std::string pre = std::string(who) + ": ";
  if (D < 0 || D > CA_LL_DMAX) { h->err = pre + "D = " + std::to_string(D) + " is outside [0, " + std::to_string(CA_LL_DMAX) + "]"; return CA_ERR_INVALID; }   // (the same on every rank: no collective)
  if (D > 0 && (!U || !V)) { h->err = pre + "D = " + std::to_string(D) + " needs both U (cells x D) and V (genes x D)"; return CA_ERR_INVALID; }
  const int64_t N = h->N; const int G = h->G, Gp = h->Gp, C = h->C, nseg = h->nseg;
  const int W = pq ? pq->W : 0;
  if (pq) {   // (the same on every rank as well)
    if (C < 2) { h->err = pre + "C = " + std::to_string(C) + " clones: a pair needs at least 2"; return CA_ERR_INVALID; }
    if (W < 1 || W > CA_PLL_WMAX) { h->err = pre + "n_weights = " + std::to_string(W) + " is outside [1, " + std::to_string(CA_PLL_WMAX) + "]"; return CA_ERR_INVALID; }
    if (!pq->weights) { h->err = pre + "weights is NULL"; return CA_ERR_INVALID; }
    for (int i = 0; i < W; ++i)
      if (!std::isfinite(pq->weights[i]) || !(pq->weights[i] > 0.0 && pq->weights[i] < 1.0)) {
        h->err = pre + "weight " + std::to_string(i) + " is " + std::to_string(pq->weights[i]) + ": not inside the open interval (0, 1)";
        return CA_ERR_INVALID;
      }
  }
  const int K = dq ? dq->K : 0, CK = C * K;
  double phi_max = 0.0;
  if (dq) {   // (the same on every rank as well)
    if (K < 1 || K > CA_DM_KMAX) { h->err = pre + "n_conc = " + std::to_string(K) + " is outside [1, " + std::to_string(CA_DM_KMAX) + "]"; return CA_ERR_INVALID; }
    if (!dq->conc) { h->err = pre + "conc is NULL"; return CA_ERR_INVALID; }
    for (int i = 0; i < K; ++i) {
      const double v = dq->conc[i];
      if (!std::isfinite(v) || !(v > 0.0)) { h->err = pre + "concentration " + std::to_string(i) + " is " + std::to_string(v) + ": not finite and > 0"; return CA_ERR_INVALID; }
      if (v > CA_DM_PHI_MAX) { h->err = pre + "concentration " + std::to_string(i) + " is above 1e300: lgamma of it overflows"; return CA_ERR_INVALID; }
      phi_max = std::max(phi_max, v);
    }
  }
  HIPCK(h, hipSetDevice(h->device));
  const int MP = C * (C - 1) / 2, MW = MP * W;
  // the sweep's table: per gene the columns [log E of the clones | V], in groups of NC columns, zero padded; where E = 0 the entry is 0 and the gene's mask has the bit
  const int ncol = C + D;
  const int NC = ncol <= 8 ? 8 : ncol <= 16 ? 16 : 32, ngrp = cdiv(ncol, NC), nct = ngrp * NC;
  std::vector<double> tab, logz0;
  std::vector<unsigned> zmask;
  std::string bad;
  if (c_lo < 0 || c_cnt < 0 || c_lo > N || c_cnt > N - c_lo)
    bad = "the cell range [" + std::to_string(c_lo) + ", " + std::to_string(c_lo) + " + " + std::to_string(c_cnt) + ") is outside [0, " + std::to_string(N) + "]";
  if (bad.empty()) bad = ll_sweep_table(h, E, V, D, NC, ngrp, tab, zmask, logz0);
  // the contraction's operands (D > 0): U and V padded to CA_LL_DMAX factors, E in groups of NZ clone columns
  const int NZ = C <= 8 ? 8 : C <= 16 ? 16 : 32, ngz = cdiv(C, NZ), nzt = ngz * NZ, nzc = cdiv(G, CA_LL_ZCHUNK);
  std::vector<double> Ut, Vt, Ez;
  if (D > 0 && bad.empty()) {
    Ut.assign((size_t)N * CA_LL_DMAX, 0.0); Vt.assign((size_t)Gp * CA_LL_DMAX, 0.0); Ez.assign((size_t)ngz * Gp * NZ, 0.0);
    for (int64_t n = 0; n < N && bad.empty(); ++n)
      for (int d = 0; d < D; ++d) {
        const double v = U[hidx(h->layout, n, d, N, D)];
        if (!std::isfinite(v)) { bad = "U has a non-finite entry (cell " + std::to_string(n) + ", factor " + std::to_string(d) + ")"; break; }
        Ut[(size_t)n * CA_LL_DMAX + d] = v;
      }
    for (int g = 0; g < G; ++g) {
      for (int d = 0; d < D; ++d) Vt[(size_t)g * CA_LL_DMAX + d] = V[hidx(h->layout, g, d, G, D)];
      for (int c = 0; c < C; ++c) Ez[((size_t)(c / NZ) * Gp + g) * NZ + c % NZ] = E[hidx(h->layout, g, c, G, C)];
    }
  }
  // the pair part's operands: E compact [G][C] for k_pair_ll (D > 0); for D = 0 the table log(A P_ga + B P_gb) of M W columns in groups of NP, its both-zero masks
  // and the slots' shifts lz = min(log Z_a, log Z_b)
  const int NP = MW <= 8 ? 8 : MW <= 16 ? 16 : 32, ngp = pq ? cdiv(MW, NP) : 0, nctp = ngp * NP;
  std::vector<double> Ec, wts, ptab, slot_lz, cv;   // (cv: the concentrations of a Dirichlet-multinomial call)
  if (dq) cv.assign(dq->conc, dq->conc + K);
  std::vector<unsigned> pzm;
  if ((pq || dq) && bad.empty()) {
    Ec.resize((size_t)G * C);
    for (int g = 0; g < G; ++g)
      for (int c = 0; c < C; ++c) Ec[(size_t)g * C + c] = E[hidx(h->layout, g, c, G, C)];
  }
  if (pq && bad.empty()) {
    wts.assign(pq->weights, pq->weights + W);
    if (D == 0) {
      ptab.assign((size_t)ngp * Gp * NP, 0.0); pzm.assign((size_t)ngp * Gp, 0u); slot_lz.assign((size_t)MW, 0.0);
      int j = 0;
      for (int a = 0; a < C; ++a)
        for (int b = a + 1; b < C; ++b)
          for (int wi = 0; wi < W; ++wi, ++j) {
            const double lz = std::min(logz0[(size_t)a], logz0[(size_t)b]), w = wts[(size_t)wi];
            const double A = w * std::exp(lz - logz0[(size_t)a]), B = (1.0 - w) * std::exp(lz - logz0[(size_t)b]);
            slot_lz[(size_t)j] = lz;
            const int grp = j / NP, jc = j % NP;
            for (int g = 0; g < G; ++g) {
              const double v = std::fma(A, Ec[(size_t)g * C + a], B * Ec[(size_t)g * C + b]);
              if (v > 0.0) ptab[((size_t)grp * Gp + g) * NP + jc] = std::log(v);
              else pzm[(size_t)grp * Gp + g] |= 1u << jc;
            }
          }
    }
  }
  if (is_sharded(h)) {   // [ranks whose input was refused]
    std::vector<double> pack{bad.empty() ? 0.0 : 1.0};
    double* scratch = nullptr;
    HIPCK(h, hipMalloc((void**)&scratch, sizeof(double)));
    const int rc = allreduce_host_vec(h, pack, scratch);
    hipFree(scratch);
    if (rc != CA_OK) return rc;
    if (pack[0] != 0.0 && bad.empty()) bad = "another rank refused its input";
  }
  if (!bad.empty()) { h->err = pre + bad; return CA_ERR_INVALID; }
  if (c_cnt == 0) return CA_OK;
  std::vector<double> lgt;
  if (with_const) { lgt.resize(CA_LL_LGTAB); for (int k = 0; k < CA_LL_LGTAB; ++k) lgt[(size_t)k] = std::lgamma((double)k + 1.0); }
  // cells in batches, so that the partial slabs stay below a quarter of a gigabyte (a cell's sums do not depend on its batch)
  const int64_t per_cell = ((int64_t)nseg * (nct + 1) + (D > 0 ? (int64_t)nzc * (nzt + 1) : 0) + (pq ? (int64_t)C + 1 + MW + (D == 0 ? (int64_t)nseg * nctp : 0) : 0) + (dq ? (int64_t)C + 1 + K + CK : 0)) * (int64_t)sizeof(double);
  const int64_t NB = std::min<int64_t>(c_cnt, std::max<int64_t>(CA_TB, (((int64_t)1 << 28) / per_cell) / CA_TB * CA_TB));
  std::vector<double> out(ll ? (size_t)c_cnt * C : 0), pout(pq && h->layout == CA_COL_MAJOR ? (size_t)c_cnt * MW : 0),
                      dout(dq && h->layout == CA_COL_MAJOR ? (size_t)c_cnt * CK : 0);
  double* const dhost = dq ? (h->layout == CA_COL_MAJOR ? dout.data() : dq->dm_ll) : nullptr;   // row-major [c_cnt][CK]
  double* const phost = pq ? (h->layout == CA_COL_MAJOR ? pout.data() : pq->pair_ll) : nullptr;   // row-major [c_cnt][MW]
  double *tab_d = nullptr, *lgt_d = nullptr, *logz_d = nullptr, *Ut_d = nullptr, *Vt_d = nullptr, *Ez_d = nullptr, *part = nullptr, *lgpart = nullptr, *zpart = nullptr, *mpart = nullptr, *ll_d = nullptr;
  double *Ec_d = nullptr, *wts_d = nullptr, *ptab_d = nullptr, *slz_d = nullptr, *lzc_d = nullptr, *base_d = nullptr, *ppart = nullptr, *pll_d = nullptr;
  double *conc_d = nullptr, *mrow_d = nullptr, *head_d = nullptr, *dll_d = nullptr;
  unsigned *zm_d = nullptr, *pzm_d = nullptr;
  auto cleanup = [&]() {
    hipFree(conc_d); hipFree(mrow_d); hipFree(head_d); hipFree(dll_d);
    hipFree(tab_d); hipFree(lgt_d); hipFree(logz_d); hipFree(Ut_d); hipFree(Vt_d); hipFree(Ez_d); hipFree(part); hipFree(lgpart); hipFree(zpart); hipFree(mpart); hipFree(ll_d); hipFree(zm_d);
    hipFree(Ec_d); hipFree(wts_d); hipFree(ptab_d); hipFree(slz_d); hipFree(lzc_d); hipFree(base_d); hipFree(ppart); hipFree(pll_d); hipFree(pzm_d);
  };
#define PCK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { h->err = std::string(#call) + ": " + hipGetErrorString(e_); cleanup(); return CA_ERR_HIP; } } while (0)
#define UP(dst, vec) do { PCK(hipMalloc((void**)&dst, (vec).size() * sizeof((vec)[0]))); PCK(hipMemcpyAsync(dst, (vec).data(), (vec).size() * sizeof((vec)[0]), hipMemcpyHostToDevice, h->stream)); } while (0)
  UP(tab_d, tab); UP(zm_d, zmask); UP(logz_d, logz0);
  if (with_const) UP(lgt_d, lgt);
  if (D > 0) { UP(Ut_d, Ut); UP(Vt_d, Vt); UP(Ez_d, Ez); }
  PCK(hipMalloc((void**)&part, (size_t)nseg * NB * nct * sizeof(double)));
  if (with_const) PCK(hipMalloc((void**)&lgpart, (size_t)nseg * NB * sizeof(double)));
  if (D > 0) {
    PCK(hipMalloc((void**)&zpart, (size_t)nzc * NB * nzt * sizeof(double)));
    PCK(hipMalloc((void**)&mpart, (size_t)nzc * NB * sizeof(double)));
  }
  PCK(hipMalloc((void**)&ll_d, (size_t)N * C * sizeof(double)));
  if (pq) {
    UP(wts_d, wts);
    if (D > 0) UP(Ec_d, Ec);
    else { UP(ptab_d, ptab); UP(pzm_d, pzm); UP(slz_d, slot_lz); PCK(hipMalloc((void**)&ppart, (size_t)nseg * NB * nctp * sizeof(double))); }
    PCK(hipMalloc((void**)&lzc_d, (size_t)NB * C * sizeof(double)));
    PCK(hipMalloc((void**)&base_d, (size_t)NB * sizeof(double)));
    PCK(hipMalloc((void**)&pll_d, (size_t)NB * MW * sizeof(double)));
  }
  if (dq) {
    UP(conc_d, cv); UP(Ec_d, Ec);
    PCK(hipMalloc((void**)&lzc_d, (size_t)NB * C * sizeof(double)));
    PCK(hipMalloc((void**)&mrow_d, (size_t)NB * sizeof(double)));
    PCK(hipMalloc((void**)&head_d, (size_t)NB * K * sizeof(double)));
    PCK(hipMalloc((void**)&dll_d, (size_t)NB * CK * sizeof(double)));
  }
  for (int64_t n_lo = c_lo; n_lo < c_lo + c_cnt; n_lo += NB) {
    const int64_t n_cnt = std::min<int64_t>(NB, c_lo + c_cnt - n_lo);
    ca_ll_ops o;
    o.tab = tab_d; o.zmask = zm_d; o.lgtab = lgt_d; o.part = part; o.lgpart = lgpart; o.n_lo = n_lo; o.n_cnt = n_cnt; o.NC = NC; o.ngrp = ngrp;
    { const int rc = launch_clone_ll(h, o); if (rc != CA_OK) { cleanup(); return rc; } }
    if (D > 0) {
      ca_llz_ops z;
      z.Ut = Ut_d; z.Vt = Vt_d; z.Ez = Ez_d; z.zpart = zpart; z.mpart = mpart; z.n_lo = n_lo; z.n_cnt = n_cnt; z.NC = NZ; z.ngrp = ngz; z.nzc = nzc;
      { const int rc = launch_clone_ll_z(h, z); if (rc != CA_OK) { cleanup(); return rc; } }
    }
    if (ll) {
      hipLaunchKernelGGL(k_clone_ll_finish, dim3((unsigned)cdiv(n_cnt * C, CA_TB)), dim3(CA_TB), 0, h->stream, part, lgpart, zpart, mpart, logz_d, Ut_d, h->s64, ll_d, n_lo, n_cnt, C,
                         (int)D, (int)nseg, nct, nzc, nzt);
      PCK(hipGetLastError());
    }
    if (pq) {
      hipLaunchKernelGGL(k_pair_cell, dim3((unsigned)cdiv(n_cnt * (C + 1), CA_TB)), dim3(CA_TB), 0, h->stream, part, lgpart, zpart, mpart, logz_d, Ut_d, h->s64, lzc_d, base_d, n_lo, n_cnt,
                         C, (int)D, (int)nseg, nct, nzc, nzt);
      PCK(hipGetLastError());
      if (D > 0) {
        ca_pll_ops p;
        p.Ec = Ec_d; p.lzc = lzc_d; p.base = base_d; p.wts = wts_d; p.out = pll_d; p.n_lo = n_lo; p.n_cnt = n_cnt; p.W = W; p.MW = MW;
        { const int rc = launch_pair_ll(h, p); if (rc != CA_OK) { cleanup(); return rc; } }
      } else {
        ca_ll_ops t;   // the table route: no lgamma sum here (base has it)
        t.tab = ptab_d; t.zmask = pzm_d; t.lgtab = nullptr; t.part = ppart; t.lgpart = nullptr; t.n_lo = n_lo; t.n_cnt = n_cnt; t.NC = NP; t.ngrp = ngp;
        { const int rc = launch_clone_ll(h, t); if (rc != CA_OK) { cleanup(); return rc; } }
        hipLaunchKernelGGL(k_pair_tab_finish, dim3((unsigned)cdiv(n_cnt * MW, CA_TB)), dim3(CA_TB), 0, h->stream, ppart, base_d, slz_d, h->s64, pll_d, n_lo, n_cnt, MW, (int)nseg, nctp);
        PCK(hipGetLastError());
      }
      PCK(hipMemcpyAsync(phost + (size_t)(n_lo - c_lo) * MW, pll_d, (size_t)n_cnt * MW * sizeof(double), hipMemcpyDeviceToHost, h->stream));   // (in stream order: before the next batch overwrites it)
    }
    if (dq) {
      hipLaunchKernelGGL(k_dm_cell, dim3((unsigned)cdiv(n_cnt * (C + K), CA_TB)), dim3(CA_TB), 0, h->stream, lgpart, zpart, mpart, logz_d, h->s64, conc_d, lzc_d, mrow_d, head_d, n_lo,
                         n_cnt, C, K, (int)D, (int)nseg, nzc, nzt);
      PCK(hipGetLastError());
      ca_dml_ops p;
      p.Ec = Ec_d; p.lzc = lzc_d; p.mrow = mrow_d; p.head = head_d; p.conc = conc_d; p.Ut = D > 0 ? Ut_d : nullptr; p.Vt = Vt_d; p.out = dll_d; p.n_lo = n_lo; p.n_cnt = n_cnt;
      p.K = K; p.CK = CK; p.ysmall = phi_max <= CA_DM_PHI_PROD ? CA_DM_YSMALL : 0;
      { const int rc = launch_dm_ll(h, p); if (rc != CA_OK) { cleanup(); return rc; } }
      PCK(hipMemcpyAsync(dhost + (size_t)(n_lo - c_lo) * CK, dll_d, (size_t)n_cnt * CK * sizeof(double), hipMemcpyDeviceToHost, h->stream));   // (in stream order: before the next batch overwrites it)
    }
  }
  if (ll) PCK(hipMemcpyAsync(out.data(), ll_d + (size_t)c_lo * C, out.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  PCK(hipStreamSynchronize(h->stream));   // (the host vectors above are read by the copies until here)
  cleanup();
#undef UP
#undef PCK
  if (ll) {
    if (h->layout == CA_COL_MAJOR) { for (int64_t n = 0; n < c_cnt; ++n) for (int c = 0; c < C; ++c) ll[hidx(h->layout, n, c, c_cnt, C)] = out[(size_t)n * C + c]; }
    else std::copy(out.begin(), out.end(), ll);
  }
  if (pq && h->layout == CA_COL_MAJOR)
    for (int64_t n = 0; n < c_cnt; ++n) for (int j = 0; j < MW; ++j) pq->pair_ll[hidx(h->layout, n, j, c_cnt, MW)] = pout[(size_t)n * MW + j];
  if (dq && h->layout == CA_COL_MAJOR)
    for (int64_t n = 0; n < c_cnt; ++n) for (int j = 0; j < CK; ++j) dq->dm_ll[hidx(h->layout, n, j, c_cnt, CK)] = dout[(size_t)n * CK + j];
  return CA_OK;
}
}  // namespace
}  // extern "C++"

int ca_clone_loglik(ca_handle h, const double* E, const double* U, const double* V, int32_t D, int32_t with_const, double* ll) {
  if (!h || !E || !ll) return CA_ERR_INVALID;
  CA_NOT_IN_RUN(h);
  return clone_ll_impl(h, "ca_clone_loglik", E, U, V, D, with_const, 0, h->N, ll, nullptr);
}

// The log-likelihood of the resident cells [cell_lo, cell_lo + cell_cnt) under every mixture of two clones and every weight of the grid (a heterotypic doublet;
// include/clonealign_hip.h has the formula and the rules).  Read-only like ca_clone_loglik, whose launches it shares; the only collective is the verdict on the input.
int ca_clone_pair_loglik(ca_handle h, const double* E, const double* U, const double* V, int32_t D, int32_t with_const, const double* weights, int32_t n_weights, int64_t cell_lo,
                         int64_t cell_cnt, double* ll, double* pair_ll) {
  if (!h) return CA_ERR_INVALID;
  if (!E || !pair_ll) { h->err = std::string("ca_clone_pair_loglik: ") + (!E ? "E" : "pair_ll") + " is NULL"; return CA_ERR_INVALID; }
  CA_NOT_IN_RUN(h);
  ca_pair_req pq{weights, (int)n_weights, pair_ll};
  return clone_ll_impl(h, "ca_clone_pair_loglik", E, U, V, D, with_const, cell_lo, cell_cnt, ll, &pq);
}

// The Dirichlet-multinomial log-likelihood of the resident cells [cell_lo, cell_lo + cell_cnt) under every clone at every concentration of the grid (overdispersed
// cell scoring; include/clonealign_hip.h has the formula and the rules, ca_k_dmll.hip.h the kernel).  Read-only like ca_clone_loglik, whose launches it shares
// (ll, the lgamma sums, log Z and the max of eta are theirs); the only collective is the verdict on the input.
int ca_clone_loglik_dm(ca_handle h, const double* E, const double* U, const double* V, int32_t D, int32_t with_const, const double* conc, int32_t n_conc, int64_t cell_lo,
                       int64_t cell_cnt, double* ll, double* dm_ll) {
  if (!h) return CA_ERR_INVALID;
  if (!E || !conc || !dm_ll) { h->err = std::string("ca_clone_loglik_dm: ") + (!E ? "E" : !conc ? "conc" : "dm_ll") + " is NULL"; return CA_ERR_INVALID; }
  CA_NOT_IN_RUN(h);
  ca_dm_req dq{conc, (int)n_conc, dm_ll};
  return clone_ll_impl(h, "ca_clone_loglik_dm", E, U, V, D, with_const, cell_lo, cell_cnt, ll, nullptr, &dq);
}

// The sufficient statistics of ca_clone_loglik by block of genes for the resident cells [cell_lo, cell_lo + cell_cnt) (include/clonealign_hip.h has the formulas and
// the rules; ca_k_blockll.hip.h the kernels).  The table, the masks and the lgamma table are ca_clone_loglik's.  The host turns the labelling into the RUN LIST
// (maximal ranges of consecutive genes with one label, cut again at the segment boundaries), the chunk list of the contraction (the same ranges cut at every
// CA_LL_ZCHUNK genes of the axis) and the lists block -> runs, block -> chunks in ascending gene order.  The slab is n_runs x cells x (C + D + 2) doubles, so the
// cell batch follows from a fixed byte budget: a chromosome-sorted axis (n_runs about n_blocks + nseg) takes the usual batch, a fully interleaved labelling
// (n_runs = G) small ones; a cell's values do not depend on its batch.  Read-only like ca_clone_loglik; the only collective is the verdict on the input.
int ca_clone_loglik_by_block(ca_handle h, const double* E, const double* U, const double* V, int32_t D, int32_t with_const, const int32_t* block_of_gene, int32_t n_blocks,
                             int64_t c_lo, int64_t c_cnt, double* A, double* logZ, double* s, double* lg) {
  if (!h) return CA_ERR_INVALID;
  const std::string pre = "ca_clone_loglik_by_block: ";
  {
    const char* null_arg = !E ? "E" : !block_of_gene ? "block_of_gene" : !A ? "A" : !logZ ? "logZ" : !s ? "s" : (with_const && !lg) ? "lg (with_const != 0)" : nullptr;
    if (null_arg) { h->err = pre + null_arg + " is NULL"; return CA_ERR_INVALID; }
  }
  CA_NOT_IN_RUN(h);
  if (D < 0 || D > CA_LL_DMAX) { h->err = pre + "D = " + std::to_string(D) + " is outside [0, " + std::to_string(CA_LL_DMAX) + "]"; return CA_ERR_INVALID; }   // (the same on every rank: no collective)
  if (D > 0 && (!U || !V)) { h->err = pre + "D = " + std::to_string(D) + " needs both U (cells x D) and V (genes x D)"; return CA_ERR_INVALID; }
  if (n_blocks < 1) { h->err = pre + "n_blocks = " + std::to_string(n_blocks) + " is below 1"; return CA_ERR_INVALID; }
  const int64_t N = h->N; const int G = h->G, Gp = h->Gp, C = h->C, nseg = h->nseg, B = n_blocks;
  for (int g = 0; g < G; ++g)
    if (block_of_gene[g] < 0 || block_of_gene[g] >= B) {
      h->err = pre + "block_of_gene[" + std::to_string(g) + "] = " + std::to_string(block_of_gene[g]) + " is outside [0, " + std::to_string(B) + ")";
      return CA_ERR_INVALID;
    }
  HIPCK(h, hipSetDevice(h->device));
  const int ncol = C + D;
  const int NC = ncol <= 8 ? 8 : ncol <= 16 ? 16 : 32, ngrp = cdiv(ncol, NC);
  std::vector<double> tab, logz0;
  std::vector<unsigned> zmask;
  std::string bad;
  if (c_lo < 0 || c_cnt < 0 || c_lo > N || c_cnt > N - c_lo)
    bad = "the cell range [" + std::to_string(c_lo) + ", " + std::to_string(c_lo) + " + " + std::to_string(c_cnt) + ") is outside [0, " + std::to_string(N) + "]";
  if (bad.empty()) bad = ll_sweep_table(h, E, V, D, NC, ngrp, tab, zmask, logz0);
  const int NZ = C <= 8 ? 8 : C <= 16 ? 16 : 32, ngz = cdiv(C, NZ);
  std::vector<double> Ut, Vt, Ez;
  if (D > 0 && bad.empty()) {
    Ut.assign((size_t)N * CA_LL_DMAX, 0.0); Vt.assign((size_t)Gp * CA_LL_DMAX, 0.0); Ez.assign((size_t)ngz * Gp * NZ, 0.0);
    for (int64_t n = 0; n < N && bad.empty(); ++n)
      for (int d = 0; d < D; ++d) {
        const double v = U[hidx(h->layout, n, d, N, D)];
        if (!std::isfinite(v)) { bad = "U has a non-finite entry (cell " + std::to_string(n) + ", factor " + std::to_string(d) + ")"; break; }
        Ut[(size_t)n * CA_LL_DMAX + d] = v;
      }
    for (int g = 0; g < G; ++g) {
      for (int d = 0; d < D; ++d) Vt[(size_t)g * CA_LL_DMAX + d] = V[hidx(h->layout, g, d, G, D)];
      for (int c = 0; c < C; ++c) Ez[((size_t)(c / NZ) * Gp + g) * NZ + c % NZ] = E[hidx(h->layout, g, c, G, C)];
    }
  }
  if (is_sharded(h)) {   // [ranks whose input was refused]
    std::vector<double> pack{bad.empty() ? 0.0 : 1.0};
    double* scratch = nullptr;
    HIPCK(h, hipMalloc((void**)&scratch, sizeof(double)));
    const int rc = allreduce_host_vec(h, pack, scratch);
    hipFree(scratch);
    if (rc != CA_OK) return rc;
    if (pack[0] != 0.0 && bad.empty()) bad = "another rank refused its input";
  }
  if (!bad.empty()) { h->err = pre + bad; return CA_ERR_INVALID; }
  if (c_cnt == 0) return CA_OK;
  // the run list and the chunk list: cuts where the label changes, and at the segment boundaries (runs) or at every CA_LL_ZCHUNK genes (chunks)
  const int segw = 64 * h->VEC;
  std::vector<int> rcut, rseg((size_t)nseg + 1, 0), zcut, run_blk, zk_blk;
  for (int g = 0; g < G; ++g) {
    const bool change = g == 0 || block_of_gene[g] != block_of_gene[g - 1];
    if (g % segw == 0) rseg[(size_t)(g / segw)] = (int)rcut.size();
    if (change || g % segw == 0) { rcut.push_back(g); run_blk.push_back(block_of_gene[g]); }
    if (change || g % CA_LL_ZCHUNK == 0) { zcut.push_back(g); zk_blk.push_back(block_of_gene[g]); }
  }
  const int n_runs = (int)rcut.size(), nzk = (int)zcut.size();
  rseg[(size_t)nseg] = n_runs;
  rcut.push_back(G); rcut.push_back(INT32_MAX);   // (the kernel reads one entry past the run it has just finished)
  zcut.push_back(G);
  // block -> its runs / chunks in ascending gene order (a counting sort keeps the order)
  auto by_block = [&](const std::vector<int>& blk, std::vector<int>& ptr, std::vector<int>& list) {
    ptr.assign((size_t)B + 1, 0); list.resize(blk.size());
    for (int b : blk) ++ptr[(size_t)b + 1];
    for (int b = 0; b < B; ++b) ptr[(size_t)b + 1] += ptr[(size_t)b];
    std::vector<int> at(ptr.begin(), ptr.end() - 1);
    for (size_t i = 0; i < blk.size(); ++i) list[(size_t)at[(size_t)blk[i]]++] = (int)i;
  };
  std::vector<int> brp, bruns, bzp, bzk;
  by_block(run_blk, brp, bruns);
  by_block(zk_blk, bzp, bzk);
  // D = 0: log Z of a block does not depend on the cell -- a float64 sum over the block's genes in ascending order, -inf where it is 0 (an empty block included)
  std::vector<double> logz0b;
  if (D == 0) {
    std::vector<double> sum((size_t)B * C, 0.0);
    for (int g = 0; g < G; ++g)
      for (int c = 0; c < C; ++c) sum[(size_t)block_of_gene[g] * C + c] += E[hidx(h->layout, g, c, G, C)];
    logz0b.resize(sum.size());
    for (size_t i = 0; i < sum.size(); ++i) logz0b[i] = sum[i] > 0.0 ? std::log(sum[i]) : -INFINITY;
  }
  std::vector<double> lgt;
  if (with_const) { lgt.resize(CA_LL_LGTAB); for (int k = 0; k < CA_LL_LGTAB; ++k) lgt[(size_t)k] = std::lgamma((double)k + 1.0); }
  // cells in batches under the byte budget: the two slabs and the batch's outputs
  const int64_t BC = (int64_t)B * C;
  const int64_t per_cell = ((int64_t)n_runs * (ncol + 2) + (D > 0 ? (int64_t)nzk * (C + 1) : 0) + 2 * BC + 2 * B) * (int64_t)sizeof(double);
  const int64_t NB = std::min<int64_t>(c_cnt, std::max<int64_t>(CA_TB, (CA_BLL_BUDGET / per_cell) / CA_TB * CA_TB));
  const bool colmaj = h->layout == CA_COL_MAJOR;
  std::vector<double> tA(colmaj ? (size_t)(c_cnt * BC) : 0), tZ(tA.size()), tS(colmaj ? (size_t)(c_cnt * B) : 0), tL(colmaj && with_const ? tS.size() : 0);
  double* const hA = colmaj ? tA.data() : A; double* const hZ = colmaj ? tZ.data() : logZ; double* const hS = colmaj ? tS.data() : s;
  double* const hL = !with_const ? nullptr : colmaj ? tL.data() : lg;   // row-major [c_cnt][...]
  double *tab_d = nullptr, *lgt_d = nullptr, *lzb_d = nullptr, *Ut_d = nullptr, *Vt_d = nullptr, *Ez_d = nullptr, *part = nullptr, *zpart = nullptr;
  double *A_d = nullptr, *Z_d = nullptr, *S_d = nullptr, *L_d = nullptr;
  unsigned* zm_d = nullptr;
  int *rcut_d = nullptr, *rseg_d = nullptr, *zcut_d = nullptr, *brp_d = nullptr, *bruns_d = nullptr, *bzp_d = nullptr, *bzk_d = nullptr;
  auto cleanup = [&]() {
    hipFree(tab_d); hipFree(lgt_d); hipFree(lzb_d); hipFree(Ut_d); hipFree(Vt_d); hipFree(Ez_d); hipFree(part); hipFree(zpart); hipFree(A_d); hipFree(Z_d); hipFree(S_d); hipFree(L_d);
    hipFree(zm_d); hipFree(rcut_d); hipFree(rseg_d); hipFree(zcut_d); hipFree(brp_d); hipFree(bruns_d); hipFree(bzp_d); hipFree(bzk_d);
  };
#define PCK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { h->err = std::string(#call) + ": " + hipGetErrorString(e_); cleanup(); return CA_ERR_HIP; } } while (0)
#define UP(dst, vec) do { PCK(hipMalloc((void**)&dst, (vec).size() * sizeof((vec)[0]))); PCK(hipMemcpyAsync(dst, (vec).data(), (vec).size() * sizeof((vec)[0]), hipMemcpyHostToDevice, h->stream)); } while (0)
  UP(tab_d, tab); UP(zm_d, zmask); UP(rcut_d, rcut); UP(rseg_d, rseg); UP(brp_d, brp); UP(bruns_d, bruns);
  if (with_const) UP(lgt_d, lgt);
  if (D > 0) { UP(Ut_d, Ut); UP(Vt_d, Vt); UP(Ez_d, Ez); UP(zcut_d, zcut); UP(bzp_d, bzp); UP(bzk_d, bzk); }
  else UP(lzb_d, logz0b);
  PCK(hipMalloc((void**)&part, (size_t)n_runs * (ncol + 2) * NB * sizeof(double)));   // (the columns in use: the padding of the last group is not stored)
  if (D > 0) PCK(hipMalloc((void**)&zpart, (size_t)nzk * (C + 1) * NB * sizeof(double)));
  PCK(hipMalloc((void**)&A_d, (size_t)(NB * BC) * sizeof(double)));
  PCK(hipMalloc((void**)&Z_d, (size_t)(NB * BC) * sizeof(double)));
  PCK(hipMalloc((void**)&S_d, (size_t)(NB * B) * sizeof(double)));
  if (with_const) PCK(hipMalloc((void**)&L_d, (size_t)(NB * B) * sizeof(double)));
  for (int64_t n_lo = c_lo; n_lo < c_lo + c_cnt; n_lo += NB) {
    const int64_t n_cnt = std::min<int64_t>(NB, c_lo + c_cnt - n_lo);
    ca_bll_ops o;
    o.tab = tab_d; o.zmask = zm_d; o.lgtab = lgt_d; o.rcut = rcut_d; o.rseg = rseg_d; o.part = part; o.n_lo = n_lo; o.n_cnt = n_cnt; o.NC = NC; o.ngrp = ngrp; o.nuse = ncol;
    { const int rc = launch_block_ll(h, o); if (rc != CA_OK) { cleanup(); return rc; } }
    if (D > 0) {
      ca_bllz_ops z;
      z.Ut = Ut_d; z.Vt = Vt_d; z.Ez = Ez_d; z.zcut = zcut_d; z.zpart = zpart; z.n_lo = n_lo; z.n_cnt = n_cnt; z.NC = NZ; z.ngrp = ngz; z.nzk = nzk;
      { const int rc = launch_block_ll_z(h, z); if (rc != CA_OK) { cleanup(); return rc; } }
    }
    hipLaunchKernelGGL(k_block_ll_finish, dim3((unsigned)cdiv(n_cnt * BC, CA_TB)), dim3(CA_TB), 0, h->stream, part, zpart, lzb_d, Ut_d, brp_d, bruns_d, bzp_d, bzk_d, A_d, Z_d, S_d, L_d,
                       n_lo, n_cnt, (int)B, C, (int)D);
    PCK(hipGetLastError());
    const size_t row = (size_t)(n_lo - c_lo);   // (the copies run in stream order: before the next batch overwrites the buffers)
    PCK(hipMemcpyAsync(hA + row * BC, A_d, (size_t)(n_cnt * BC) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    PCK(hipMemcpyAsync(hZ + row * BC, Z_d, (size_t)(n_cnt * BC) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    PCK(hipMemcpyAsync(hS + row * B, S_d, (size_t)(n_cnt * B) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (with_const) PCK(hipMemcpyAsync(hL + row * B, L_d, (size_t)(n_cnt * B) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  }
  PCK(hipStreamSynchronize(h->stream));   // (the host vectors above are read by the copies until here)
  cleanup();
#undef UP
#undef PCK
  if (colmaj)
    for (int64_t n = 0; n < c_cnt; ++n) {
      for (int64_t j = 0; j < BC; ++j) { A[hidx(h->layout, n, j, c_cnt, BC)] = tA[(size_t)(n * BC + j)]; logZ[hidx(h->layout, n, j, c_cnt, BC)] = tZ[(size_t)(n * BC + j)]; }
      for (int b = 0; b < B; ++b) { s[hidx(h->layout, n, b, c_cnt, B)] = tS[(size_t)(n * B + b)]; if (with_const) lg[hidx(h->layout, n, b, c_cnt, B)] = tL[(size_t)(n * B + b)]; }
    }
  return CA_OK;
}

// Per-cell MAP psi and the clone posterior at it for the resident cells under a fit's gene-level parameters (include/clonealign_hip.h has the algorithm and the
// rules).  ONE sweep over the matrix (k_clone_ll against [log E | V]: A, B and the constant), then rounds of two launches that never read it, queued back to
// back; every few rounds the host reads the frozen flags and stops queuing when no cell is left -- freezing is per cell, so WHEN the host looks changes no
// result.  Read-only like ca_clone_loglik; a sharded handle takes part in ONE small collective, the verdict on the input.
int ca_project_cells(ca_handle h, const double* E, const double* V, int32_t K, int32_t P, const double* X, const double* log_prior, const double* psi_start,
                     int32_t with_const, int32_t max_iter, double tol, double max_step, double* psi, double* ll, double* clone_probs, double* objective,
                     int32_t* rounds, uint8_t* converged) {
  if (!h || !E || !ll || !clone_probs || !objective || !rounds || !converged || (K > 0 && !psi)) return CA_ERR_INVALID;
  CA_NOT_IN_RUN(h);
  const int D = K + P;
  auto refuse = [&](const std::string& why) { h->err = "ca_project_cells: " + why; return CA_ERR_INVALID; };   // (these are the same on every rank: no collective)
  if (K < 0 || K > CA_PROJ_KMAX) return refuse("K = " + std::to_string(K) + " is outside [0, " + std::to_string(CA_PROJ_KMAX) + "] (the device limit of the moment kernel)");
  if (P < 0 || D > CA_LL_DMAX) return refuse("K + P = " + std::to_string(D) + " is outside [0, " + std::to_string(CA_LL_DMAX) + "]");
  if (D > 0 && !V) return refuse("K + P = " + std::to_string(D) + " needs V (genes x (K + P))");
  if (P > 0 && !X) return refuse("P = " + std::to_string(P) + " needs X (cells x P)");
  if (max_iter < 0) return refuse("max_iter = " + std::to_string(max_iter) + " is negative");
  if (!(tol > 0.0) || !std::isfinite(tol)) return refuse("tol = " + std::to_string(tol) + " is not a positive finite number");
  if (!(max_step > 0.0) || !std::isfinite(max_step)) return refuse("max_step = " + std::to_string(max_step) + " is not a positive finite number");
  const int poll_set = (with_const >> 8) & 0xFF, poll = poll_set ? poll_set : 4;   // rounds between two looks at the frozen flags (255: practically never)
  const bool lgc = (with_const & 1) != 0;
  HIPCK(h, hipSetDevice(h->device));
  const int64_t N = h->N; const int G = h->G, Gp = h->Gp, C = h->C, nseg = h->nseg;
  const int ncol = C + D;
  const int NC = ncol <= 8 ? 8 : ncol <= 16 ? 16 : 32, ngrp = cdiv(ncol, NC), nct = ngrp * NC;
  std::vector<double> tab, logz0;
  std::vector<unsigned> zmask;
  std::string bad = ll_sweep_table(h, E, V, D, NC, ngrp, tab, zmask, logz0);
  // the moments' operands: U = [psi | x] and V padded to CA_LL_DMAX factors, E in groups of NZ clone columns
  const int NM = 1 + K + K * (K + 1) / 2;
  const int NZ = (K <= 1 && C > 8) ? 16 : 8, ngz = cdiv(C, NZ), nmt = ngz * NZ * NM, nzc = cdiv(G, CA_LL_ZCHUNK);
  std::vector<double> Ut((size_t)N * CA_LL_DMAX, 0.0), Vt((size_t)Gp * CA_LL_DMAX, 0.0), Ez((size_t)ngz * Gp * NZ, 0.0), lp;
  for (int64_t n = 0; n < N && bad.empty(); ++n) {
    for (int k = 0; k < K && psi_start; ++k) {
      const double v = psi_start[hidx(h->layout, n, k, N, K)];
      if (!std::isfinite(v)) { bad = "psi_start has a non-finite entry (cell " + std::to_string(n) + ", factor " + std::to_string(k) + ")"; break; }
      Ut[(size_t)n * CA_LL_DMAX + k] = v;
    }
    for (int p = 0; p < P && bad.empty(); ++p) {
      const double v = X[hidx(h->layout, n, p, N, P)];
      if (!std::isfinite(v)) { bad = "X has a non-finite entry (cell " + std::to_string(n) + ", covariate " + std::to_string(p) + ")"; break; }
      Ut[(size_t)n * CA_LL_DMAX + K + p] = v;
    }
  }
  if (log_prior && bad.empty()) {
    lp.resize((size_t)N * C);
    for (int64_t n = 0; n < N && bad.empty(); ++n)
      for (int c = 0; c < C; ++c) {
        const double v = log_prior[hidx(h->layout, n, c, N, C)];
        if (std::isnan(v) || v == HUGE_VAL) { bad = "log_prior has a NaN or +inf entry (cell " + std::to_string(n) + ", clone " + std::to_string(c) + "); -inf excludes a clone"; break; }
        lp[(size_t)n * C + c] = v;
      }
  }
  if (bad.empty())
    for (int g = 0; g < G; ++g) {
      for (int d = 0; d < D; ++d) Vt[(size_t)g * CA_LL_DMAX + d] = V[hidx(h->layout, g, d, G, D)];
      for (int c = 0; c < C; ++c) Ez[((size_t)(c / NZ) * Gp + g) * NZ + c % NZ] = E[hidx(h->layout, g, c, G, C)];
    }
  if (is_sharded(h)) {   // [ranks whose input was refused]
    std::vector<double> pack{bad.empty() ? 0.0 : 1.0};
    double* scratch = nullptr;
    HIPCK(h, hipMalloc((void**)&scratch, sizeof(double)));
    const int rc = allreduce_host_vec(h, pack, scratch);
    hipFree(scratch);
    if (rc != CA_OK) return rc;
    if (pack[0] != 0.0 && bad.empty()) bad = "another rank refused its input";
  }
  if (!bad.empty()) return refuse(bad);
  if (N == 0) return CA_OK;
  std::vector<double> lgt;
  if (lgc) { lgt.resize(CA_LL_LGTAB); for (int k = 0; k < CA_LL_LGTAB; ++k) lgt[(size_t)k] = std::lgamma((double)k + 1.0); }
  // cells in batches, so that the partial slabs stay below a quarter of a gigabyte (a cell's results do not depend on its batch)
  const int64_t per_cell = ((int64_t)nseg * (nct + 1) + (int64_t)nzc * (nmt + 1)) * (int64_t)sizeof(double);
  const int64_t NB = std::min<int64_t>(N, std::max<int64_t>(CA_TB, (((int64_t)1 << 28) / per_cell) / CA_TB * CA_TB));
  std::vector<double> o_ll((size_t)N * C), o_pr((size_t)N * C), o_u((size_t)N * CA_LL_DMAX);
  std::vector<unsigned char> fr((size_t)NB);
  double *tab_d = nullptr, *lgt_d = nullptr, *Ut_d = nullptr, *Vt_d = nullptr, *Ez_d = nullptr, *lp_d = nullptr, *part = nullptr, *lgpart = nullptr, *zpart = nullptr, *mpart = nullptr,
         *A_d = nullptr, *B_d = nullptr, *ll_d = nullptr, *pr_d = nullptr, *obj_d = nullptr;
  unsigned* zm_d = nullptr; unsigned char *fr_d = nullptr, *cv_d = nullptr; int* rd_d = nullptr;
  auto cleanup = [&]() { hipFree(tab_d); hipFree(lgt_d); hipFree(Ut_d); hipFree(Vt_d); hipFree(Ez_d); hipFree(lp_d); hipFree(part); hipFree(lgpart); hipFree(zpart); hipFree(mpart);
                         hipFree(A_d); hipFree(B_d); hipFree(ll_d); hipFree(pr_d); hipFree(obj_d); hipFree(zm_d); hipFree(fr_d); hipFree(cv_d); hipFree(rd_d); };
#define PCK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { h->err = std::string(#call) + ": " + hipGetErrorString(e_); cleanup(); return CA_ERR_HIP; } } while (0)
#define UP(dst, vec) do { PCK(hipMalloc((void**)&dst, (vec).size() * sizeof((vec)[0]))); PCK(hipMemcpyAsync(dst, (vec).data(), (vec).size() * sizeof((vec)[0]), hipMemcpyHostToDevice, h->stream)); } while (0)
  UP(tab_d, tab); UP(zm_d, zmask); UP(Ut_d, Ut); UP(Vt_d, Vt); UP(Ez_d, Ez);
  if (lgc) UP(lgt_d, lgt);
  if (log_prior) UP(lp_d, lp);
  PCK(hipMalloc((void**)&part, (size_t)nseg * NB * nct * sizeof(double)));
  if (lgc) PCK(hipMalloc((void**)&lgpart, (size_t)nseg * NB * sizeof(double)));
  PCK(hipMalloc((void**)&zpart, (size_t)nzc * NB * nmt * sizeof(double)));
  PCK(hipMalloc((void**)&mpart, (size_t)nzc * NB * sizeof(double)));
  PCK(hipMalloc((void**)&A_d, (size_t)N * C * sizeof(double)));
  PCK(hipMalloc((void**)&B_d, (size_t)N * CA_LL_DMAX * sizeof(double)));
  PCK(hipMalloc((void**)&ll_d, (size_t)N * C * sizeof(double)));
  PCK(hipMalloc((void**)&pr_d, (size_t)N * C * sizeof(double)));
  PCK(hipMalloc((void**)&obj_d, (size_t)N * sizeof(double)));
  PCK(hipMalloc((void**)&fr_d, (size_t)N));
  PCK(hipMalloc((void**)&cv_d, (size_t)N));
  PCK(hipMalloc((void**)&rd_d, (size_t)N * sizeof(int)));
  PCK(hipMemsetAsync(B_d, 0, (size_t)N * CA_LL_DMAX * sizeof(double), h->stream));   // (the padding factors)
  PCK(hipMemsetAsync(fr_d, 0, (size_t)N, h->stream));
  for (int64_t n_lo = 0; n_lo < N; n_lo += NB) {
    const int64_t n_cnt = std::min<int64_t>(NB, N - n_lo);
    ca_ll_ops o;
    o.tab = tab_d; o.zmask = zm_d; o.lgtab = lgt_d; o.part = part; o.lgpart = lgpart; o.n_lo = n_lo; o.n_cnt = n_cnt; o.NC = NC; o.ngrp = ngrp;
    { const int rc = launch_clone_ll(h, o); if (rc != CA_OK) { cleanup(); return rc; } }
    hipLaunchKernelGGL(k_proj_sums, dim3((unsigned)cdiv(n_cnt * ncol, CA_TB)), dim3(CA_TB), 0, h->stream, part, lgpart, h->s64, A_d, B_d, n_lo, n_cnt, C, D, (int)nseg, nct);
    PCK(hipGetLastError());
    ca_pm_ops m;
    m.Ut = Ut_d; m.Vt = Vt_d; m.Ez = Ez_d; m.frozen = fr_d; m.zpart = zpart; m.mpart = mpart; m.n_lo = n_lo; m.n_cnt = n_cnt; m.K = K; m.NC = NZ; m.ngrp = ngz; m.nzc = nzc;
    ca_ps_ops s;
    s.zpart = zpart; s.mpart = mpart; s.A = A_d; s.B = B_d; s.lp = lp_d; s.Ut = Ut_d; s.frozen = fr_d; s.conv = cv_d; s.rounds = rd_d; s.ll = ll_d; s.probs = pr_d; s.obj = obj_d;
    s.n_lo = n_lo; s.n_cnt = n_cnt; s.K = K; s.nzc = nzc; s.nmt = nmt; s.final = 0; s.tol = tol; s.max_step = max_step;
    bool all_frozen = false;
    for (int t = 0; K > 0 && t < max_iter && !all_frozen; ++t) {
      s.round = t;
      { const int rc = launch_proj_mom(h, m); if (rc != CA_OK) { cleanup(); return rc; } }
      { const int rc = launch_proj_step(h, s); if (rc != CA_OK) { cleanup(); return rc; } }
      if ((t + 1) % poll == 0 && t + 1 < max_iter) {
        PCK(hipMemcpyAsync(fr.data(), fr_d + n_lo, (size_t)n_cnt, hipMemcpyDeviceToHost, h->stream));
        PCK(hipStreamSynchronize(h->stream));
        all_frozen = std::find(fr.begin(), fr.begin() + n_cnt, (unsigned char)0) == fr.begin() + n_cnt;
      }
    }
    if (!all_frozen) {   // the cells that never froze (all of them when K = 0 or max_iter = 0): ll and the posterior at the psi they hold
      s.round = K > 0 ? max_iter : 0; s.final = 1;
      { const int rc = launch_proj_mom(h, m); if (rc != CA_OK) { cleanup(); return rc; } }
      { const int rc = launch_proj_step(h, s); if (rc != CA_OK) { cleanup(); return rc; } }
    }
  }
  std::vector<int> o_rd((size_t)N);
  PCK(hipMemcpyAsync(o_ll.data(), ll_d, o_ll.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  PCK(hipMemcpyAsync(o_pr.data(), pr_d, o_pr.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  PCK(hipMemcpyAsync(o_u.data(), Ut_d, o_u.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  PCK(hipMemcpyAsync(objective, obj_d, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  PCK(hipMemcpyAsync(o_rd.data(), rd_d, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  PCK(hipMemcpyAsync(converged, cv_d, (size_t)N, hipMemcpyDeviceToHost, h->stream));
  PCK(hipStreamSynchronize(h->stream));   // (the host vectors above are read by the copies until here)
  cleanup();
#undef UP
#undef PCK
  for (int64_t n = 0; n < N; ++n) {
    rounds[n] = o_rd[(size_t)n];
    for (int c = 0; c < C; ++c) { ll[hidx(h->layout, n, c, N, C)] = o_ll[(size_t)n * C + c]; clone_probs[hidx(h->layout, n, c, N, C)] = o_pr[(size_t)n * C + c]; }
    for (int k = 0; k < K; ++k) psi[hidx(h->layout, n, k, N, K)] = o_u[(size_t)n * CA_LL_DMAX + k];
  }
  return CA_OK;
}

// The clone evidence with psi integrated out, per resident cell and clone (include/clonealign_hip.h has the algorithm and the rules; ca_k_evidence.hip.h the
// kernels).  ONE sweep over the matrix, ca_project_cells' (k_clone_ll against [log E | V], k_proj_sums: A, B and the constant); then per batch of cells Newton
// rounds of two launches (k_ev_mom with all moments, k_ev_step) that never read it, queued back to back with the host looking at the pairs' states every few
// rounds -- freezing is per (cell, clone), so WHEN the host looks changes no result -- and the quadrature: k_ev_nodes, ONE k_ev_mom over the (clone, node) slots
// (Z0 only), k_ev_reduce.  K = 0 is ca_clone_loglik itself.  Read-only; a sharded handle takes part in ONE small collective, the verdict on the input.
int ca_clone_evidence(ca_handle h, const double* E, const double* V, int32_t K, int32_t P, const double* X, const double* psi_start, int32_t with_const,
                      int32_t n_nodes, const double* nodes, const double* weights, int32_t max_iter, double tol, double max_step, double* evidence, double* laplace,
                      double* psi_mode, double* psi_prec, int32_t* rounds, uint8_t* converged) {
  if (!h || !E || !evidence || !laplace || !rounds || !converged || (K > 0 && (!psi_mode || !psi_prec))) return CA_ERR_INVALID;
  CA_NOT_IN_RUN(h);
  const int D = K + P, Q = n_nodes;
  auto refuse = [&](const std::string& why) { h->err = "ca_clone_evidence: " + why; return CA_ERR_INVALID; };   // (these are the same on every rank: no collective)
  if (K < 0 || K > CA_PROJ_KMAX) return refuse("K = " + std::to_string(K) + " is outside [0, " + std::to_string(CA_PROJ_KMAX) + "] (the device limit of the moment kernel)");
  if (P < 0 || D > CA_LL_DMAX) return refuse("K + P = " + std::to_string(D) + " is outside [0, " + std::to_string(CA_LL_DMAX) + "]");
  if (D > 0 && !V) return refuse("K + P = " + std::to_string(D) + " needs V (genes x (K + P))");
  if (P > 0 && !X) return refuse("P = " + std::to_string(P) + " needs X (cells x P)");
  if (max_iter < 0) return refuse("max_iter = " + std::to_string(max_iter) + " is negative");
  if (!(tol > 0.0) || !std::isfinite(tol)) return refuse("tol = " + std::to_string(tol) + " is not a positive finite number");
  if (!(max_step > 0.0) || !std::isfinite(max_step)) return refuse("max_step = " + std::to_string(max_step) + " is not a positive finite number");
  if (Q < 1 || Q > CA_EV_QMAX) return refuse("n_nodes = " + std::to_string(Q) + " is outside [1, " + std::to_string(CA_EV_QMAX) + "]");
  if (!nodes && K > 0) return refuse("nodes is NULL (n_nodes x K)");
  if (!weights) return refuse("weights is NULL (n_nodes)");
  {
    double wsum = 0.0;
    for (int q = 0; q < Q; ++q) {
      for (int k = 0; k < K; ++k)
        if (!std::isfinite(nodes[(size_t)q * K + k])) return refuse("node " + std::to_string(q) + " has a non-finite coordinate (factor " + std::to_string(k) + ")");
      if (!std::isfinite(weights[q]) || !(weights[q] > 0.0)) return refuse("weight " + std::to_string(q) + " is " + std::to_string(weights[q]) + ": not positive and finite");
      wsum += weights[q];
    }
    if (!(std::fabs(wsum - 1.0) <= 1e-12)) return refuse("the weights sum to " + std::to_string(wsum) + ": off 1 by more than 1e-12");
  }
  const int poll_set = (with_const >> 8) & 0xFF, poll = poll_set ? poll_set : 4;   // rounds between two looks at the pairs' states (255: practically never)
  const bool lgc = (with_const & 1) != 0;
  const int64_t N = h->N; const int G = h->G, Gp = h->Gp, C = h->C, nseg = h->nseg;
  if (K == 0) {   // nothing to integrate: ca_clone_loglik's value, bit for bit (its launches, its collective)
    std::vector<double> ll((size_t)N * C + 1);
    const int rc = clone_ll_impl(h, "ca_clone_evidence", E, X, V, P, lgc ? 1 : 0, 0, N, ll.data(), nullptr);
    if (rc != CA_OK) return rc;
    for (int64_t n = 0; n < N; ++n)
      for (int c = 0; c < C; ++c) {
        const size_t i = hidx(h->layout, n, c, N, C);
        evidence[i] = laplace[i] = ll[i];
        rounds[i] = 0;
        converged[i] = ll[i] > -HUGE_VAL ? 1 : 0;
      }
    return CA_OK;
  }
  HIPCK(h, hipSetDevice(h->device));
  const int ncol = C + D;
  const int NC = ncol <= 8 ? 8 : ncol <= 16 ? 16 : 32, ngrp = cdiv(ncol, NC), nct = ngrp * NC;
  std::vector<double> tab, logz0;
  std::vector<unsigned> zmask;
  std::string bad = ll_sweep_table(h, E, V, D, NC, ngrp, tab, zmask, logz0);
  const int NM = 1 + K + K * (K + 1) / 2, NH = K * (K + 1) / 2, nzc = cdiv(G, CA_LL_ZCHUNK), CQ = C * Q;
  std::vector<double> Ut((size_t)N * CA_LL_DMAX, 0.0), Vt((size_t)Gp * CA_LL_DMAX, 0.0), Ec((size_t)Gp * C, 0.0);   // U = [start | x]
  for (int64_t n = 0; n < N && bad.empty(); ++n) {
    for (int k = 0; k < K && psi_start; ++k) {
      const double v = psi_start[hidx(h->layout, n, k, N, K)];
      if (!std::isfinite(v)) { bad = "psi_start has a non-finite entry (cell " + std::to_string(n) + ", factor " + std::to_string(k) + ")"; break; }
      Ut[(size_t)n * CA_LL_DMAX + k] = v;
    }
    for (int p = 0; p < P && bad.empty(); ++p) {
      const double v = X[hidx(h->layout, n, p, N, P)];
      if (!std::isfinite(v)) { bad = "X has a non-finite entry (cell " + std::to_string(n) + ", covariate " + std::to_string(p) + ")"; break; }
      Ut[(size_t)n * CA_LL_DMAX + K + p] = v;
    }
  }
  if (bad.empty())
    for (int g = 0; g < G; ++g) {
      for (int d = 0; d < D; ++d) Vt[(size_t)g * CA_LL_DMAX + d] = V[hidx(h->layout, g, d, G, D)];
      for (int c = 0; c < C; ++c) Ec[(size_t)g * C + c] = E[hidx(h->layout, g, c, G, C)];
    }
  if (is_sharded(h)) {   // [ranks whose input was refused]
    std::vector<double> pack{bad.empty() ? 0.0 : 1.0};
    double* scratch = nullptr;
    HIPCK(h, hipMalloc((void**)&scratch, sizeof(double)));
    const int rc = allreduce_host_vec(h, pack, scratch);
    hipFree(scratch);
    if (rc != CA_OK) return rc;
    if (pack[0] != 0.0 && bad.empty()) bad = "another rank refused its input";
  }
  if (!bad.empty()) return refuse(bad);
  if (N == 0) return CA_OK;
  std::vector<double> lgt, nd(nodes, nodes + (size_t)Q * K), wt(weights, weights + Q);
  if (lgc) { lgt.resize(CA_LL_LGTAB); for (int k = 0; k < CA_LL_LGTAB; ++k) lgt[(size_t)k] = std::lgamma((double)k + 1.0); }
  // cells in batches, so that the partial slabs stay below a quarter of a gigabyte (a cell's results do not depend on its batch)
  const int zcols = std::max(C * NM, CQ), mcols = CQ;   // (one pair of slabs serves the rounds and the quadrature pass)
  const int64_t per_cell = ((int64_t)nseg * (nct + 1) + (int64_t)nzc * (zcols + mcols) + (int64_t)CQ * K + (int64_t)C * (K + NH + 5)) * (int64_t)sizeof(double);
  const int64_t NB = std::min<int64_t>(N, std::max<int64_t>(CA_TB, (((int64_t)1 << 28) / per_cell) / CA_TB * CA_TB));
  std::vector<double> b_ev((size_t)NB * C), b_lap((size_t)NB * C), b_ps((size_t)NB * C * K), b_H((size_t)NB * C * NH);
  std::vector<int> b_rd((size_t)NB * C);
  std::vector<unsigned char> b_cv((size_t)NB * C), fr((size_t)NB * C);
  double *tab_d = nullptr, *lgt_d = nullptr, *Ut_d = nullptr, *Vt_d = nullptr, *Ec_d = nullptr, *nd_d = nullptr, *wt_d = nullptr, *part = nullptr, *lgpart = nullptr, *zpart = nullptr,
         *mpart = nullptr, *A_d = nullptr, *B_d = nullptr, *ps_d = nullptr, *pq_d = nullptr, *fs_d = nullptr, *H_d = nullptr, *lap_d = nullptr, *ev_d = nullptr;
  unsigned* zm_d = nullptr; unsigned char *fz_d = nullptr, *cv_d = nullptr; int* rd_d = nullptr;
  auto cleanup = [&]() { hipFree(tab_d); hipFree(lgt_d); hipFree(Ut_d); hipFree(Vt_d); hipFree(Ec_d); hipFree(nd_d); hipFree(wt_d); hipFree(part); hipFree(lgpart); hipFree(zpart);
                         hipFree(mpart); hipFree(A_d); hipFree(B_d); hipFree(ps_d); hipFree(pq_d); hipFree(fs_d); hipFree(H_d); hipFree(lap_d); hipFree(ev_d); hipFree(zm_d);
                         hipFree(fz_d); hipFree(cv_d); hipFree(rd_d); };
#define PCK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { h->err = std::string(#call) + ": " + hipGetErrorString(e_); cleanup(); return CA_ERR_HIP; } } while (0)
#define UP(dst, vec) do { PCK(hipMalloc((void**)&dst, (vec).size() * sizeof((vec)[0]))); PCK(hipMemcpyAsync(dst, (vec).data(), (vec).size() * sizeof((vec)[0]), hipMemcpyHostToDevice, h->stream)); } while (0)
  UP(tab_d, tab); UP(zm_d, zmask); UP(Ut_d, Ut); UP(Vt_d, Vt); UP(Ec_d, Ec); UP(nd_d, nd); UP(wt_d, wt);
  if (lgc) UP(lgt_d, lgt);
  PCK(hipMalloc((void**)&part, (size_t)nseg * NB * nct * sizeof(double)));
  if (lgc) PCK(hipMalloc((void**)&lgpart, (size_t)nseg * NB * sizeof(double)));
  PCK(hipMalloc((void**)&zpart, (size_t)nzc * NB * zcols * sizeof(double)));
  PCK(hipMalloc((void**)&mpart, (size_t)nzc * NB * mcols * sizeof(double)));
  PCK(hipMalloc((void**)&A_d, (size_t)N * C * sizeof(double)));
  PCK(hipMalloc((void**)&B_d, (size_t)N * CA_LL_DMAX * sizeof(double)));
  PCK(hipMalloc((void**)&ps_d, (size_t)NB * C * K * sizeof(double)));
  PCK(hipMalloc((void**)&pq_d, (size_t)NB * CQ * K * sizeof(double)));
  PCK(hipMalloc((void**)&fs_d, (size_t)NB * C * sizeof(double)));
  PCK(hipMalloc((void**)&H_d, (size_t)NB * C * NH * sizeof(double)));
  PCK(hipMalloc((void**)&lap_d, (size_t)NB * C * sizeof(double)));
  PCK(hipMalloc((void**)&ev_d, (size_t)NB * C * sizeof(double)));
  PCK(hipMalloc((void**)&fz_d, (size_t)NB * C));
  PCK(hipMalloc((void**)&cv_d, (size_t)NB * C));
  PCK(hipMalloc((void**)&rd_d, (size_t)NB * C * sizeof(int)));
  PCK(hipMemsetAsync(B_d, 0, (size_t)N * CA_LL_DMAX * sizeof(double), h->stream));   // (the padding factors)
  for (int64_t n_lo = 0; n_lo < N; n_lo += NB) {
    const int64_t n_cnt = std::min<int64_t>(NB, N - n_lo);
    ca_ll_ops o;
    o.tab = tab_d; o.zmask = zm_d; o.lgtab = lgt_d; o.part = part; o.lgpart = lgpart; o.n_lo = n_lo; o.n_cnt = n_cnt; o.NC = NC; o.ngrp = ngrp;
    { const int rc = launch_clone_ll(h, o); if (rc != CA_OK) { cleanup(); return rc; } }
    hipLaunchKernelGGL(k_proj_sums, dim3((unsigned)cdiv(n_cnt * ncol, CA_TB)), dim3(CA_TB), 0, h->stream, part, lgpart, h->s64, A_d, B_d, n_lo, n_cnt, C, D, (int)nseg, nct);
    PCK(hipGetLastError());
    ca_evm_ops m;
    m.Ut = Ut_d; m.Vt = Vt_d; m.Ec = Ec_d; m.ps = ps_d; m.fz = fz_d; m.zpart = zpart; m.mpart = mpart; m.n_lo = n_lo; m.n_cnt = n_cnt; m.K = K; m.Q = 1; m.nslot = C; m.nzc = nzc;
    m.full = true;
    ca_evs_ops s;
    s.zpart = zpart; s.mpart = mpart; s.A = A_d; s.B = B_d; s.Ut = Ut_d; s.nodes = nd_d; s.wts = wt_d; s.ps = ps_d; s.pq = pq_d; s.fz = fz_d; s.conv = cv_d; s.rounds = rd_d;
    s.fstar = fs_d; s.Hm = H_d; s.lap = lap_d; s.ev = ev_d; s.n_lo = n_lo; s.n_cnt = n_cnt; s.K = K; s.Q = Q; s.nzc = nzc; s.round = 0; s.final = 0; s.tol = tol; s.max_step = max_step;
    { const int rc = launch_ev_fin(h, s, CA_EV_INIT); if (rc != CA_OK) { cleanup(); return rc; } }
    bool all_frozen = false;
    for (int t = 0; t < max_iter && !all_frozen; ++t) {
      s.round = t;
      { const int rc = launch_ev_mom(h, m); if (rc != CA_OK) { cleanup(); return rc; } }
      { const int rc = launch_ev_fin(h, s, CA_EV_STEP); if (rc != CA_OK) { cleanup(); return rc; } }
      if ((t + 1) % poll == 0 && t + 1 < max_iter) {
        PCK(hipMemcpyAsync(fr.data(), fz_d, (size_t)n_cnt * C, hipMemcpyDeviceToHost, h->stream));
        PCK(hipStreamSynchronize(h->stream));
        all_frozen = std::find(fr.begin(), fr.begin() + n_cnt * C, (unsigned char)CA_EV_LIVE) == fr.begin() + n_cnt * C;
      }
    }
    if (!all_frozen) {   // the pairs that never froze (all of them when max_iter = 0): f and H at the psi they hold
      s.round = max_iter; s.final = 1;
      { const int rc = launch_ev_mom(h, m); if (rc != CA_OK) { cleanup(); return rc; } }
      { const int rc = launch_ev_fin(h, s, CA_EV_STEP); if (rc != CA_OK) { cleanup(); return rc; } }
    }
    // the quadrature: the nodes' psi, Z0 of every (clone, node) slot in one launch, the reduction over the nodes
    { const int rc = launch_ev_fin(h, s, CA_EV_NODES); if (rc != CA_OK) { cleanup(); return rc; } }
    m.ps = pq_d; m.Q = Q; m.nslot = CQ; m.full = false;
    { const int rc = launch_ev_mom(h, m); if (rc != CA_OK) { cleanup(); return rc; } }
    { const int rc = launch_ev_fin(h, s, CA_EV_REDUCE); if (rc != CA_OK) { cleanup(); return rc; } }
    const size_t nc = (size_t)n_cnt * C;
    PCK(hipMemcpyAsync(b_ev.data(), ev_d, nc * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    PCK(hipMemcpyAsync(b_lap.data(), lap_d, nc * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    PCK(hipMemcpyAsync(b_ps.data(), ps_d, nc * K * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    PCK(hipMemcpyAsync(b_H.data(), H_d, nc * NH * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    PCK(hipMemcpyAsync(b_rd.data(), rd_d, nc * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    PCK(hipMemcpyAsync(b_cv.data(), cv_d, nc, hipMemcpyDeviceToHost, h->stream));
    PCK(hipStreamSynchronize(h->stream));
    for (int64_t li = 0; li < n_cnt; ++li) {   // the batch's slabs are [column][cell]
      const int64_t n = n_lo + li;
      for (int c = 0; c < C; ++c) {
        const size_t i = hidx(h->layout, n, c, N, C), j = (size_t)c * n_cnt + li;
        evidence[i] = b_ev[j]; laplace[i] = b_lap[j]; rounds[i] = b_rd[j]; converged[i] = b_cv[j];
        for (int k = 0; k < K; ++k) psi_mode[hidx(h->layout, n, c * K + k, N, C * K)] = b_ps[((size_t)c * K + k) * n_cnt + li];
        for (int k = 0; k < NH; ++k) psi_prec[hidx(h->layout, n, c * NH + k, N, C * NH)] = b_H[((size_t)c * NH + k) * n_cnt + li];
      }
    }
  }
  cleanup();
#undef UP
#undef PCK
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
      double* scratch = nullptr;
      HIPCK(h, hipMalloc((void**)&scratch, pack.size() * sizeof(double)));
      const int rc = allreduce_host_vec(h, pack, scratch);
      hipFree(scratch);
      if (rc != CA_OK) return rc;
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
  int2* list_d = nullptr; ca_mse_row* meta = nullptr; ca_lx_blk* blk_d = nullptr; int* first_d = nullptr; double *inv_d = nullptr, *part1 = nullptr, *part2 = nullptr, *sums_d = nullptr;
  auto cleanup = [&]() { hipFree(list_d); hipFree(meta); hipFree(blk_d); hipFree(first_d); hipFree(inv_d); hipFree(part1); hipFree(part2); hipFree(sums_d); };
#define PCK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { h->err = std::string(#call) + ": " + hipGetErrorString(e_); cleanup(); return CA_ERR_HIP; } } while (0)
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
    PCK(hipMalloc((void**)&list_d, (size_t)M * sizeof(int2)));
    PCK(hipMalloc((void**)&meta, (size_t)M * sizeof(ca_mse_row)));
    PCK(hipMalloc((void**)&blk_d, blk.size() * sizeof(ca_lx_blk)));
    PCK(hipMalloc((void**)&first_d, first.size() * sizeof(int)));
    PCK(hipMalloc((void**)&inv_d, (size_t)M * sizeof(double)));
    PCK(hipMalloc((void**)&part1, (size_t)o.nrg * Gp * sizeof(double)));
    PCK(hipMalloc((void**)&part2, (size_t)o.nrg * Gp * sizeof(double)));
    PCK(hipMalloc((void**)&sums_d, sums.size() * sizeof(double)));
    PCK(hipMemcpyAsync(list_d, list.data(), (size_t)M * sizeof(int2), hipMemcpyHostToDevice, h->stream));
    PCK(hipMemcpyAsync(inv_d, sf.data(), (size_t)M * sizeof(double), hipMemcpyHostToDevice, h->stream));
    PCK(hipMemcpyAsync(blk_d, blk.data(), blk.size() * sizeof(ca_lx_blk), hipMemcpyHostToDevice, h->stream));
    PCK(hipMemcpyAsync(first_d, first.data(), first.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_lx_prep, dim3(cdiv(M, CA_TB)), dim3(CA_TB), 0, h->stream, list_d, inv_d, h->n_ovf > 0 ? h->ovf_rowptr : nullptr, meta, M);
    PCK(hipGetLastError());
    o.meta = meta; o.blk = blk_d; o.part1 = part1; o.part2 = part2;
    { const int rc = launch_logexpr(h, o); if (rc != CA_OK) { cleanup(); return rc; } }
    hipLaunchKernelGGL(k_lx_finish, dim3(cdiv(Gp, 64), Q + 1), dim3(1024), 0, h->stream, part1, part2, first_d, Q, Gp, sums_d);
    PCK(hipGetLastError());
    PCK(hipMemcpyAsync(sums.data(), sums_d, sums.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    PCK(hipStreamSynchronize(h->stream));   // (the host vectors above are read by the copies until here)
    cleanup();
  }
#undef PCK
  std::vector<double> cnt((size_t)Q, 0.0);
  if (bad.empty()) for (int q = 0; q < Q; ++q) cnt[(size_t)q] = (double)(start[(size_t)q + 1] - start[(size_t)q]);
  if (is_sharded(h)) {   // totals over all ranks: [S1 Q x G | S2 G | cells per group Q | ranks whose input was refused]
    std::vector<double> pack;
    pack.reserve((size_t)(Q + 1) * G + Q + 1);
    for (int q = 0; q <= Q; ++q) pack.insert(pack.end(), sums.begin() + (size_t)q * Gp, sums.begin() + (size_t)q * Gp + G);
    pack.insert(pack.end(), cnt.begin(), cnt.end());
    pack.push_back(bad.empty() ? 0.0 : 1.0);
    double* scratch = nullptr;
    HIPCK(h, hipMalloc((void**)&scratch, pack.size() * sizeof(double)));
    const int rc = allreduce_host_vec(h, pack, scratch);
    hipFree(scratch);
    if (rc != CA_OK) return rc;
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
