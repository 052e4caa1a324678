// ca_eng_init.inc -- part of clonealign_hip.hip (textually included there, in this order; one translation unit): C ABI, once per fit on the resident matrix: PCA initialisation of psi (transformed count-matrix pass, Gram-Schmidt and Jacobi on the host, blocked subspace iteration), per-clone gene sums.
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

