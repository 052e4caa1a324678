// ca_eng_separability.inc -- part of clonealign_hip.hip (textually included there, after ca_eng_predmom.inc; one translation unit; ca_gen_call, the call's scaffold, is defined in ca_eng_simulate.inc): C ABI without a handle: per cell and ordered pair of clones the per-read moments of the log-likelihood ratio and the probability of a read that excludes the rival, in closed form (ca_clone_separability; include/clonealign_hip.h states the outputs), the kernel time of the calling thread's last call.
namespace { thread_local double sep_kernel_ms = 0.0; }

int ca_clone_separability_kernel_ms(double* ms) { return gen_kernel_ms(ms, sep_kernel_ms); }

// How a call with factors is cut: W columns of the right-hand side at a time (B [Gp][W] within 48 MB; all ncolp where they fit) and NB cells per batch (the
// slab part [nzc][NB][W] within 128 MB, the merged rows R [NB][ncolp] and the outputs [NB][C + 4 C C] within 32 MB each, never more than CA_SEP_NB cells; at least 16,
// one row tile, whatever that takes).  Both depend on (G, C) alone and change no bit: a cell's values come from its own row of the product.
#define CA_SEP_NB 65536
extern "C++" {
namespace {
struct ca_sep_cut { int Gp, nzc, ncol, ncolp, W; int64_t NB; };
inline ca_sep_cut sep_cut(int32_t G, int32_t C) {
  ca_sep_cut k;
  k.Gp = (G + 63) / 64 * 64;
  k.nzc = cdiv(G, CA_LL_ZCHUNK);
  k.ncol = C + 4 * C * (C - 1);
  k.ncolp = (k.ncol + 15) / 16 * 16;
  const int64_t wmax = std::max<int64_t>(16, (((int64_t)48 << 20) / ((int64_t)k.Gp * 8)) / 16 * 16);
  k.W = (int)std::min<int64_t>(k.ncolp, wmax);
  const int64_t by_part = ((int64_t)128 << 20) / ((int64_t)k.nzc * k.W * 8), by_row = ((int64_t)32 << 20) / ((int64_t)k.ncolp * 8);
  k.NB = std::max<int64_t>(16, std::min<int64_t>(CA_SEP_NB, std::min(by_part, by_row)));
  return k;
}
// one cell's row of the five outputs without factors, from the per-gene sums themselves (p = e / Z, d = delta - Delta): e [G][C] normalised
void sep_row_host(const std::vector<double>& e, int G, int C, double* logZ, double* excl, double* m1, double* m2, double* m3) {
  std::vector<double> le((size_t)G * C), Z((size_t)C, 0.0);
  for (int g = 0; g < G; ++g)
    for (int c = 0; c < C; ++c) {
      const double v = e[(size_t)g * C + c];
      le[(size_t)g * C + c] = v > 0.0 ? std::log(v) : 0.0;
      Z[(size_t)c] += v;
    }
  for (int c = 0; c < C; ++c) logZ[c] = std::log(Z[(size_t)c]);
  for (int a = 0; a < C; ++a)
    for (int b = 0; b < C; ++b) {
      double x = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
      if (a != b) {
        const double dl = logZ[a] - logZ[b];
        for (int g = 0; g < G; ++g) {
          const double ea = e[(size_t)g * C + a], eb = e[(size_t)g * C + b];
          if (!(ea > 0.0)) continue;
          const double p = ea / Z[(size_t)a];
          if (!(eb > 0.0)) { x += p; continue; }
          const double d = (le[(size_t)g * C + a] - le[(size_t)g * C + b]) - dl;
          s1 += p * d; s2 += p * (d * d); s3 += p * (d * d * d);
        }
      }
      excl[a * C + b] = x; m1[a * C + b] = s1; m2[a * C + b] = s2; m3[a * C + b] = s3;
    }
}
}  // namespace
}  // extern "C++"

// Validates everything on the host before the first byte of an output is written.  D = 0: one row on the host, copied to every cell.  D > 0: k_sep_loge once;
// the right-hand side once where all columns fit one chunk, else per batch and chunk; per batch of cells and chunk of columns the product and k_sep_merge
// (k_sep_scale once a batch: the shifts are the same for every chunk of columns), then k_sep_finish and the batch's five copies to the caller.
int ca_clone_separability(int64_t N, int32_t G, int32_t C, int32_t D, const double* E, const double* V, const double* U, int32_t device, double* logZ, double* excl,
                          double* m1, double* m2, double* m3, char* err) {
  ca_gen_call call("ca_clone_separability", err, sep_kernel_ms);
  if (N < 0 || G < 1 || C < 2) return call.refuse("N = " + std::to_string(N) + ", G = " + std::to_string(G) + ", C = " + std::to_string(C) + ": N must be >= 0, G >= 1 and C >= 2");
  if (D < 0 || D > CA_LL_DMAX) return call.refuse("D = " + std::to_string(D) + " is outside [0, " + std::to_string(CA_LL_DMAX) + "]");
  if (D > 0 && (!U || !V)) return call.refuse("D = " + std::to_string(D) + " needs both U (cells x D) and V (genes x D)");
  if (!E) return call.refuse("E must not be NULL");
  const std::pair<const char*, double*> outs[5] = {{"logZ", logZ}, {"excl", excl}, {"m1", m1}, {"m2", m2}, {"m3", m3}};
  for (const auto& o : outs)
    if (!o.second) return call.refuse(std::string(o.first) + " must not be NULL");
  if ((double)N * (double)C * (double)C >= 1152921504606846976.0) return call.refuse("N x C x C = " + std::to_string(N) + " x " + std::to_string(C) + " x " + std::to_string(C) + " is 2^60 or more");
  const ca_sep_cut cut = sep_cut(G, C);
  // e = E / its column sum (genes ascending), [Gp][C] with zero rows past G
  std::vector<double> colsum((size_t)C, 0.0), Ec((size_t)cut.Gp * C, 0.0);
  for (int g = 0; g < G; ++g)
    for (int c = 0; c < C; ++c) {
      const double v = E[(size_t)g * C + c];
      if (!std::isfinite(v) || v < 0.0) return call.refuse("E has a negative or non-finite entry (gene " + std::to_string(g) + ", clone " + std::to_string(c) + ")");
      colsum[(size_t)c] += v;
    }
  for (int c = 0; c < C; ++c) {
    if (colsum[(size_t)c] == 0.0) return call.refuse("E is zero in every gene of clone " + std::to_string(c) + ": its column sums to 0");
    if (!std::isfinite(colsum[(size_t)c])) return call.refuse("E sums to a non-finite value in clone " + std::to_string(c));
  }
  for (int g = 0; g < G; ++g)
    for (int c = 0; c < C; ++c) Ec[(size_t)g * C + c] = E[(size_t)g * C + c] / colsum[(size_t)c];
  std::vector<double> Vt((size_t)(D > 0 ? cut.Gp : 0) * CA_LL_DMAX, 0.0);
  for (int g = 0; g < G && D > 0; ++g)
    for (int d = 0; d < D; ++d) {
      const double v = V[(size_t)g * D + d];
      if (!std::isfinite(v)) return call.refuse("V has a non-finite entry (gene " + std::to_string(g) + ", factor " + std::to_string(d) + ")");
      Vt[(size_t)g * CA_LL_DMAX + d] = v;
    }
  for (int64_t n = 0; n < N && D > 0; ++n)
    for (int d = 0; d < D; ++d)
      if (!std::isfinite(U[(size_t)n * D + d])) return call.refuse("U has a non-finite entry (cell " + std::to_string(n) + ", factor " + std::to_string(d) + ")");
  if (N == 0) return CA_OK;
  const size_t CC = (size_t)C * C;

  if (D == 0) {
    sep_row_host(Ec, G, C, logZ, excl, m1, m2, m3);
    for (int64_t n = 1; n < N; ++n) {
      std::copy(logZ, logZ + C, logZ + (size_t)n * C);
      for (double* p : {excl, m1, m2, m3}) std::copy(p, p + CC, p + (size_t)n * CC);
    }
    return CA_OK;
  }

  const int64_t NB = std::min<int64_t>(N, cut.NB);
  const bool one_chunk = cut.W == cut.ncolp;
  call.open(device);
  ca_sep_ops o;
  o.G = G; o.Gp = cut.Gp; o.C = C; o.nzc = cut.nzc; o.ncol = cut.ncol; o.ncolp = cut.ncolp;
  o.Ec = call.upload(Ec); o.Vt = call.upload(Vt);
  o.lE = call.alloc<double>((int64_t)cut.Gp * C);
  o.B = call.alloc<double>((int64_t)cut.Gp * cut.W);
  double* Ut_d = call.alloc<double>(NB * CA_LL_DMAX);
  o.Ut = Ut_d;
  o.part = call.alloc<double>((int64_t)cut.nzc * NB * cut.W);
  o.mpart = call.alloc<double>((int64_t)cut.nzc * NB); o.wk = call.alloc<double>((int64_t)cut.nzc * NB); o.m = call.alloc<double>(NB);
  o.R = call.alloc<double>(NB * cut.ncolp);
  o.logZ = call.alloc<double>(NB * C);
  double* pair_d = call.alloc<double>(4 * NB * (int64_t)CC);
  if (call.rc != CA_OK) return call.failed();
  if (!call.timed([&]() { return launch_sep_loge(call.stream, o); })) return call.failed();
  o.c_lo = 0; o.W = cut.W;
  if (one_chunk && !call.timed([&]() { return launch_sep_build(call.stream, o); })) return call.failed();
  std::vector<double> Ut((size_t)NB * CA_LL_DMAX, 0.0);
  for (int64_t n_lo = 0; n_lo < N; n_lo += NB) {
    const int64_t n_cnt = std::min<int64_t>(NB, N - n_lo);
    for (int64_t i = 0; i < n_cnt; ++i)
      for (int d = 0; d < D; ++d) Ut[(size_t)i * CA_LL_DMAX + d] = U[(size_t)(n_lo + i) * D + d];
    if (!call.note(hipMemcpyAsync(Ut_d, Ut.data(), (size_t)n_cnt * CA_LL_DMAX * sizeof(double), hipMemcpyHostToDevice, call.stream), "hipMemcpyAsync of U") ||
        !call.note(hipStreamSynchronize(call.stream), "hipStreamSynchronize"))   // (the copy has read the staging vector)
      return call.failed();
    o.n_cnt = n_cnt;
    o.excl = pair_d; o.m1 = pair_d + n_cnt * (int64_t)CC; o.m2 = pair_d + 2 * n_cnt * (int64_t)CC; o.m3 = pair_d + 3 * n_cnt * (int64_t)CC;
    for (int c_lo = 0; c_lo < cut.ncolp; c_lo += cut.W) {
      o.c_lo = c_lo; o.W = std::min(cut.W, cut.ncolp - c_lo);
      if (!one_chunk && !call.timed([&]() { return launch_sep_build(call.stream, o); })) return call.failed();
      if (!call.timed([&]() { return launch_sep_prod(call.stream, o); })) return call.failed();
      if (c_lo == 0 && !call.timed([&]() { return launch_sep_scale(call.stream, o); })) return call.failed();
      if (!call.timed([&]() { return launch_sep_merge(call.stream, o); })) return call.failed();
    }
    if (!call.timed([&]() { return launch_sep_finish(call.stream, o); })) return call.failed();
    const size_t zb = (size_t)n_cnt * C * sizeof(double), pb = (size_t)n_cnt * CC * sizeof(double);
    double* const dst[4] = {excl, m1, m2, m3};
    if (!call.ok(hipMemcpy(logZ + (size_t)n_lo * C, o.logZ, zb, hipMemcpyDeviceToHost), "hipMemcpy", zb)) return call.failed();
    for (int k = 0; k < 4; ++k)
      if (!call.ok(hipMemcpy(dst[k] + (size_t)n_lo * CC, pair_d + (size_t)k * n_cnt * CC, pb, hipMemcpyDeviceToHost), "hipMemcpy", pb)) return call.failed();
  }
  return call.done();
}
