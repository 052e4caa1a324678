// ca_k_separability.hip.h -- part of ca_kernels.hip.h (textually included there, after ca_k_predmom.hip.h): how well expression separates every ordered pair of
// clones, per cell, IN CLOSED FORM (ca_clone_separability; include/clonealign_hip.h states the outputs).  For a row drawn from clone a the log-likelihood
// ratio against clone b is a linear statistic of one multinomial; its per-read moments are sums over the genes of functions of p_nag.  With factors all
// ordered pairs of all cells are ONE DENSE FLOAT64 PRODUCT, cells x columns over the genes, with exp(eta - m) as the left operand: the product
// ca_clone_loglik_reweighted runs for its log Z side, so it runs on that kernel -- k_boot_prod<float, true, NT> of ca_k_bootll.hip.h, unchanged (v_mfma_f64_16x16x4_f64,
// the shift per chunk of CA_LL_ZCHUNK genes, part[chunk][cell][column] and mpart[chunk][cell]).  New here: its right-hand side, the merge and the epilogue.
//   k_sep_loge    log e once per (gene, clone), 0 where e = 0: every later log e is a load, none is taken per pair.
//   k_sep_build   the right-hand side B[Gp][W] for the columns [c_lo, c_lo + W) of the call's ncol = C + 4 C (C - 1): column c < C is e_gc; the ordered pair
//                 (a, b), a != b, has index p = a (C - 1) + (b < a ? b : b - 1) and owns the columns C + 4 p + k: k = 0 e_ga 1[X], k = 1, 2, 3 e_ga 1[S] delta^k with
//                 delta = log e_ga - log e_gb, S = {e_ga > 0 and e_gb > 0}, X = {e_ga > 0 and e_gb = 0}.  Rows g >= G and columns past ncol are 0.
//   k_sep_scale   per cell: m = the max of the gene chunks' shifts, wk[chunk][cell] = exp(m_chunk - m) -- once a batch, not once a column.
//   k_sep_merge   per (cell, column): R[cell][column] = sum over the chunks, ascending, of part wk (one fma a chunk).  The moment columns are signed, so the
//                 merge is linear; ca_ll_logz's log form is for positive sums only.
//   k_sep_finish  per (cell, a, b): log Z and the four pair values from the merged row by the expanded forms (below); the diagonal and every pair with an
//                 underflowed Z are exactly 0 -- the mask is looked at before anything is divided.
// Every sum has a fixed order and there are no atomics: two calls agree bit for bit.  An output element of an MFMA depends on its own row of A and column of B
// alone, so a cell's values depend neither on its place in a tile or batch nor on which chunk of columns a column went with.

__global__ void __launch_bounds__(CA_TB) k_sep_loge(const double* __restrict__ Ec /*[Gp][C]*/, double* __restrict__ lE /*[Gp][C]*/, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * CA_TB + threadIdx.x;
  if (i >= n) return;
  const double e = Ec[i];
  lE[i] = e > 0.0 ? log(e) : 0.0;
}

__global__ void __launch_bounds__(CA_TB) k_sep_build(const double* __restrict__ Ec /*[Gp][C]: e, rows g >= G zero*/, const double* __restrict__ lE /*[Gp][C]*/,
                                                     double* __restrict__ B /*[Gp][W]*/, int c_lo, int W, int ncol, int G, int Gp, int C) {
  const int64_t i = (int64_t)blockIdx.x * CA_TB + threadIdx.x;
  if (i >= (int64_t)Gp * W) return;
  const int g = (int)(i / W), col = c_lo + (int)(i - (int64_t)g * W);
  double v = 0.0;
  if (g < G && col < ncol) {
    const double* __restrict__ er = Ec + (int64_t)g * C;
    if (col < C) v = er[col];
    else {
      const int p = (col - C) >> 2, k = (col - C) & 3;
      const int a = p / (C - 1), r = p - a * (C - 1), b = r + (r >= a ? 1 : 0);
      const double ea = er[a], eb = er[b];
      if (ea > 0.0) {
        if (k == 0) v = eb > 0.0 ? 0.0 : ea;
        else if (eb > 0.0) {
          const double d = lE[(int64_t)g * C + a] - lE[(int64_t)g * C + b];
          v = ea * (k == 1 ? d : k == 2 ? d * d : d * d * d);
        }
      }
    }
  }
  B[i] = v;
}

__global__ void __launch_bounds__(CA_TB) k_sep_scale(const double* __restrict__ mpart /*[nzc][n_cnt]*/, double* __restrict__ wk /*[nzc][n_cnt]*/, double* __restrict__ m /*[n_cnt]*/,
                                                     int64_t n_cnt, int nzc) {
  const int64_t li = (int64_t)blockIdx.x * CA_TB + threadIdx.x;
  if (li >= n_cnt) return;
  const double mx = ca_ll_chunk_max(mpart + li, n_cnt, nullptr, 0, nzc);   // (every chunk holds a gene: finite)
  for (int k = 0; k < nzc; ++k) wk[(int64_t)k * n_cnt + li] = exp(mpart[(int64_t)k * n_cnt + li] - mx);
  m[li] = mx;
}

__global__ void __launch_bounds__(CA_TB) k_sep_merge(const double* __restrict__ part /*[nzc][n_cnt][W]*/, const double* __restrict__ wk /*[nzc][n_cnt]*/,
                                                     double* __restrict__ R /*[n_cnt][ncolp]*/, int64_t n_cnt, int nzc, int c_lo, int W, int ncolp) {
  const int64_t i = (int64_t)blockIdx.x * CA_TB + threadIdx.x;
  if (i >= n_cnt * W) return;
  const int64_t li = i / W;
  const int j = (int)(i - li * W);
  double z = 0.0;
  for (int k = 0; k < nzc; ++k) z = fma(part[(int64_t)k * n_cnt * W + i], wk[(int64_t)k * n_cnt + li], z);
  R[li * ncolp + c_lo + j] = z;
}

// With Z_c = R[c], X = R[C + 4 p], M_k = R[C + 4 p + k]:  Delta = log Z_a - log Z_b,  excl = X / Z_a,  q = 1 - excl,  r_k = M_k / Z_a,
//   m1 = r_1 - Delta q,  m2 = r_2 - 2 Delta r_1 + Delta^2 q,  m3 = r_3 - 3 Delta r_2 + 3 Delta^2 r_1 - Delta^3 q.
// Columns a and b equal bit for bit: Z_a = Z_b (the same sums in the same order), Delta = 0 and every M_k a sum of zeros -- exactly 0.
__global__ void __launch_bounds__(CA_TB) k_sep_finish(const double* __restrict__ R /*[n_cnt][ncolp]*/, const double* __restrict__ m /*[n_cnt]*/, double* __restrict__ logZ /*[n_cnt][C]*/,
                                                      double* __restrict__ excl, double* __restrict__ m1, double* __restrict__ m2, double* __restrict__ m3 /*[n_cnt][C][C]*/,
                                                      int64_t n_cnt, int C, int ncolp) {
  const int64_t i = (int64_t)blockIdx.x * CA_TB + threadIdx.x;
  if (i >= n_cnt * C * C) return;
  const int64_t li = i / ((int64_t)C * C);
  const int ab = (int)(i - li * C * C), a = ab / C, b = ab - a * C;
  const double* __restrict__ r = R + li * ncolp;
  const double za = r[a], zb = r[b];
  double x = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
  if (a == b) logZ[li * C + a] = m[li] + log(za);   // (Z = 0: -inf, no NaN -- m is finite)
  else if (za > 0.0 && zb > 0.0) {
    const double* __restrict__ q4 = r + C + 4 * (a * (C - 1) + (b < a ? b : b - 1));
    const double dl = za == zb ? 0.0 : log(za) - log(zb);
    x = q4[0] / za;
    const double q = 1.0 - x, r1 = q4[1] / za, r2 = q4[2] / za, r3 = q4[3] / za;
    v1 = r1 - dl * q;
    v2 = r2 - 2.0 * dl * r1 + dl * dl * q;
    v3 = r3 - 3.0 * dl * r2 + 3.0 * dl * dl * r1 - dl * dl * dl * q;
  }
  excl[i] = x; m1[i] = v1; m2[i] = v2; m3[i] = v3;
}
