// ca_k_bootll.hip.h -- part of ca_kernels.hip.h (textually included there, in this order): the gene-reweighted log-likelihood of the resident count matrix
// (ca_clone_loglik_reweighted; bootstrap support for clone calls).  In the notation of ca_k_loglik.hip.h, for replicate weights w[r][g] >= 0:
//   A_r[n][c] = sum_g w_rg xlogy(y_ng, E_gc),  s_r[n] = sum_g w_rg y_ng,  Z_r[n][c] = sum_g w_rg E_gc exp(eta_ng),  ll_r[n][c] = A_r[n][c] - s_r[n] log Z_r[n][c]
// (sum_g w_rg y_ng eta_ng and the lgamma constant are the same for every clone and are left out).
//
// All replicates of a chunk are TWO DENSE FLOAT64 PRODUCTS with the cells as rows, the (replicate, clone) pairs as columns and the genes as the inner dimension,
// so they run on v_mfma_f64_16x16x4_f64: a wave owns 16 cells and NT <= CA_BOOT_NT column tiles of 16, the accumulators (8 VGPRs a tile) are all it keeps.
//   k_boot_build      the chunk's right-hand sides: B1[g][r (C + 1) + c] = w_rg log E_gc (0 where E = 0), column r (C + 1) + C = w_rg;  B2[g][r C + c] = w_rg E_gc;
//                     rows g >= G and columns past the chunk are 0.  At D = 0 no second product runs: Z0[r][c] = sum_g w_rg E_gc, g ascending, by the last block.
//   k_boot_prod<YT, EXPSRC, NT>   ONE template, two sources of the left operand.  EXPSRC = false: the resident row in its own storage (u8 + overflow list, u16,
//                     f32), 16 bytes a lane, widened to float64 in registers -- exact; an escaped u8 count is patched to its true value there.  EXPSRC = true:
//                     exp(eta_ng - m) from Ut, Vt with m the max of eta over the gene chunk for that cell (ca_ll_zchunk's shift: every gene of the chunk
//                     counts, whatever its weight -- a zero weight behaves as E = 0 does in ca_clone_loglik).
//                     Lane l holds A[row = l & 15][k = l >> 4] and B[k = l >> 4][column = l & 15]; C/D is the f64 map, row = (l >> 4) + 4 reg, column = l & 15.
//                     Which gene is k of which step is free as long as both operands agree: a lane reads VEC consecutive genes of its row at gene
//                     base + (l >> 4) VEC and step j takes the j-th of them.  The gene axis is cut into chunks of CA_LL_ZCHUNK; a wave adds its chunk's genes
//                     in that fixed order into part[chunk][cell][column] (and the chunk's m into mpart[chunk][cell]).
//   k_boot_zero<YT>   the -inf pattern: over the host-built list of genes where some E_gc = 0 only, a thread per (cell, replicate, 32 clones) ors the mask of
//                     the clones with E = 0 wherever the weight and the count are both positive.  No second full-width product.
//   k_boot_finish     per (cell, replicate): the chunks added in ascending order (A, s), the chunks of Z merged in ascending order under their overall max
//                     (ca_ll_logz), ll_r = -inf where the mask says so, else A - s log Z for s > 0, else 0.  No NaN: the mask is looked at before anything is
//                     subtracted, so -inf - s (-inf) is never formed, and s = 0 never meets log Z = -inf.
//   k_boot_reduce     per cell, the chunk's replicates in ascending order: t = ll_r + log_prior, its argmax (ties to the lowest clone) into votes, softmax_c(t)
//                     and its square added into prob_sum / prob_sq.  A running sum from the first replicate to the last: where the chunks are cut changes nothing.
// Every sum has a fixed order and there are no atomics: two calls agree bit for bit.  An output element of an MFMA depends on its own row of A and column of B
// alone, so a cell's values depend neither on its place in a tile or batch nor on the column its replicate landed in.
#define CA_BOOT_NT 8   // most column tiles of 16 per wave: 64 accumulator VGPRs (the instantiations: 4 and 8).  Twelve and sixteen tiles -- the 18 tiles of 32 replicates x
                       // (8 clones + 1) as 2 x 9, the 16 of the exponent product as 1 x 16, one exp per (cell, gene) and chunk -- were built and measured SLOWER
                       // (100k x 5k x 8, R = 100: kernels 178.9 ms against 137.1): at 160 - 208 VGPRs two waves a SIMD no longer hide the loads of the right-hand side

typedef double ca_f64x4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(CA_TB) k_boot_build(const double* __restrict__ Ec /*[Gp][C]*/, const double* __restrict__ W /*[R][G]*/, double* __restrict__ B1 /*[Gp][nc1]*/,
                                                      double* __restrict__ B2 /*[Gp][nc2], or null: D = 0*/, double* __restrict__ Z0 /*[rc][C]: D = 0*/, int r0, int rc, int G, int Gp,
                                                      int C, int nc1, int nc2, int nb_tab) {
  if ((int)blockIdx.x >= nb_tab) {   // D = 0: Z0[r][c], a thread per pair, the genes in ascending order
    const int i = ((int)blockIdx.x - nb_tab) * CA_TB + (int)threadIdx.x;
    if (i >= rc * C) return;
    const int r = i / C, c = i - r * C;
    const double* __restrict__ wr = W + (int64_t)(r0 + r) * G;
    double z = 0.0;
    for (int g = 0; g < G; ++g) z = fma(wr[g], Ec[(int64_t)g * C + c], z);
    Z0[i] = z;
    return;
  }
  const int64_t n1 = (int64_t)Gp * nc1, n2 = B2 ? (int64_t)Gp * nc2 : 0;
  const int64_t i = (int64_t)blockIdx.x * CA_TB + threadIdx.x;
  if (i < n1) {
    const int g = (int)(i / nc1), col = (int)(i - (int64_t)g * nc1);
    const int r = col / (C + 1), c = col - r * (C + 1);
    double v = 0.0;
    if (g < G && r < rc) {
      const double w = W[(int64_t)(r0 + r) * G + g];
      if (c == C) v = w;
      else { const double e = Ec[(int64_t)g * C + c]; v = e > 0.0 ? w * log(e) : 0.0; }
    }
    B1[i] = v;
  } else if (i < n1 + n2) {
    const int64_t k = i - n1;
    const int g = (int)(k / nc2), col = (int)(k - (int64_t)g * nc2);
    const int r = col / C, c = col - r * C;
    B2[k] = (g < G && r < rc) ? W[(int64_t)(r0 + r) * G + g] * Ec[(int64_t)g * C + c] : 0.0;
  }
}

// grid: (row tiles of 16 cells / waves per block, gene chunks, groups of NT column tiles)
template <typename YT, bool EXPSRC, int NT>
__global__ void __launch_bounds__(CA_TB) k_boot_prod(const YT* __restrict__ Y, const int64_t* __restrict__ orowptr /* or null */, const int* __restrict__ ocol,
                                                     const float* __restrict__ oval, const double* __restrict__ Ut /*[N][CA_LL_DMAX]*/, const double* __restrict__ Vt /*[Gp][CA_LL_DMAX]*/,
                                                     const double* __restrict__ B /*[Gp][ncol]*/, double* __restrict__ part /*[nzc][n_cnt][ncol]*/,
                                                     double* __restrict__ mpart /*[nzc][n_cnt]: EXPSRC*/, int64_t n_lo, int64_t n_cnt, int G, int Gp, int ncol) {
  constexpr int VEC = EXPSRC ? 1 : YVec<YT>::VEC;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t row0 = ((int64_t)blockIdx.x * (CA_TB / 64) + wave) * 16;
  if (row0 >= n_cnt) return;   // (wave-uniform; the kernel has no block barrier)
  const int r16 = lane & 15, kq = lane >> 4;
  const int64_t li = row0 + r16;
  const int64_t n = n_lo + (li < n_cnt ? li : n_cnt - 1);   // (a lane past the end reads the last cell; its rows are not stored)
  const int zc = blockIdx.y;
  const int g_lo = zc * CA_LL_ZCHUNK, g_hi = (g_lo + CA_LL_ZCHUNK < G) ? g_lo + CA_LL_ZCHUNK : G;
  const int tile0 = (int)blockIdx.z * NT;
  const int nt = (ncol / 16 - tile0 < NT) ? ncol / 16 - tile0 : NT;
  const double* __restrict__ bcol = B + (int64_t)tile0 * 16 + r16;
  ca_f64x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = (ca_f64x4){0.0, 0.0, 0.0, 0.0};
  // one step: this lane's gene g of its row with value a against the NT column tiles
  auto step = [&](double a, int g) {
    const double* __restrict__ br = bcol + (int64_t)g * ncol;
#pragma unroll
    for (int t = 0; t < NT; ++t)
      if (t < nt) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, br[t * 16], acc[t], 0, 0, 0);   // (wave-uniform test)
  };
  double m = 0.0;
  if constexpr (EXPSRC) {
    double u[CA_LL_DMAX];
#pragma unroll
    for (int d = 0; d < CA_LL_DMAX; ++d) u[d] = Ut[n * CA_LL_DMAX + d];
    m = -__builtin_inf();
    for (int g = g_lo + kq; g < g_hi; g += 4) m = fmax(m, ca_ll_eta(u, Vt + (int64_t)g * CA_LL_DMAX));
    m = fmax(m, __shfl_xor(m, 16));
    m = fmax(m, __shfl_xor(m, 32));   // (the chunk holds at least one gene: finite)
    for (int gb = g_lo; gb < g_hi; gb += 4) {
      const int g = gb + kq;   // (g < Gp: the tables are padded to Gp rows, a multiple of 64)
      const double a = g < g_hi ? exp(ca_ll_eta(u, Vt + (int64_t)g * CA_LL_DMAX) - m) : 0.0;
      step(a, g);
    }
  } else {
    typedef unsigned v4u_ __attribute__((ext_vector_type(4)));
    long long oe0 = 0; int noe = 0;
    if constexpr (sizeof(YT) == 1) {
      if (orowptr) { oe0 = orowptr[n]; noe = (int)(orowptr[n + 1] - oe0); }
    }
    const YT* __restrict__ yrow = Y + n * (int64_t)Gp + kq * VEC;
    for (int gb = g_lo; gb < g_hi; gb += 4 * VEC) {   // (gb + 4 VEC <= Gp: rows are padded to a multiple of 64 VEC)
      const v4u_ t_ = *reinterpret_cast<const v4u_*>(yrow + gb);
      float y[VEC];
      YVec<YT>::decode((uint4){t_.x, t_.y, t_.z, t_.w}, y);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const int g = gb + kq * VEC + j;
        double a = (double)y[j];
        if constexpr (sizeof(YT) == 1) {
          if (y[j] == 255.f && noe > 0) a += ca_mse_excess(ocol, oval, oe0, noe, g);   // per lane, rare: 255 + an entry of the overflow list
        }
        step(g < g_hi ? a : 0.0, g);
      }
    }
  }
  // C/D of the f64 MFMA: row = (lane >> 4) + 4 reg, column = lane & 15
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (t < nt) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t lo = row0 + kq + 4 * q;
        if (lo < n_cnt) part[((int64_t)zc * n_cnt + lo) * ncol + (int64_t)(tile0 + t) * 16 + r16] = acc[t][q];
      }
    }
  }
  if constexpr (EXPSRC) {
    if (blockIdx.z == 0 && kq == 0 && li < n_cnt) mpart[(int64_t)zc * n_cnt + li] = m;
  }
}

// the -inf pattern of a chunk: flags[(cell, replicate)][word] |= the E = 0 clones of every listed gene whose weight and count are both positive
template <typename YT>
__global__ void __launch_bounds__(CA_TB) k_boot_zero(const YT* __restrict__ Y, const double* __restrict__ W /*[R][G]*/, const int* __restrict__ zg /*[nz]*/,
                                                     const unsigned* __restrict__ zm /*[nz][nw]*/, unsigned* __restrict__ flags /*[n_cnt][rcp][nw]*/, int64_t n_lo, int64_t n_cnt,
                                                     int r0, int rc, int rcp, int nw, int nz, int G, int Gp) {
  const int64_t i = (int64_t)blockIdx.x * CA_TB + threadIdx.x;
  if (i >= n_cnt * rc * nw) return;
  const int wd = (int)(i % nw);
  const int64_t q = i / nw;
  const int r = (int)(q % rc);
  const int64_t li = q / rc;
  const YT* __restrict__ yrow = Y + (n_lo + li) * (int64_t)Gp;
  const double* __restrict__ wr = W + (int64_t)(r0 + r) * G;
  unsigned f = 0u;
  for (int k = 0; k < nz; ++k) {
    const int g = zg[k];
    if (wr[g] > 0.0 && (float)yrow[g] > 0.f) f |= zm[(int64_t)k * nw + wd];   // (an escaped u8 count is stored as 255: positive either way)
  }
  flags[(li * rcp + r) * nw + wd] = f;
}

__global__ void __launch_bounds__(CA_TB) k_boot_finish(const double* __restrict__ part /*[nzc][n_cnt][nc1]*/, const double* __restrict__ zpart /*[nzc][n_cnt][nc2]: D > 0*/,
                                                       const double* __restrict__ mpart /*[nzc][n_cnt]: D > 0*/, const double* __restrict__ Z0 /*[rc][C]: D = 0*/,
                                                       const unsigned* __restrict__ flags /*[n_cnt][rcp][nw], or null*/, double* __restrict__ llb /*[n_cnt][rc][C]*/,
                                                       double* __restrict__ sb /*[n_cnt][rc]*/, int64_t n_cnt, int rc, int rcp, int nw, int C, int D, int nzc, int nc1, int nc2) {
  const int64_t i = (int64_t)blockIdx.x * CA_TB + threadIdx.x;
  if (i >= n_cnt * rc) return;
  const int64_t li = i / rc;
  const int r = (int)(i - li * rc);
  const double* __restrict__ p1 = part + li * nc1 + (int64_t)r * (C + 1);
  const double s = ca_ll_colsum(p1 + C, n_cnt * nc1, nullptr, 0, nzc);
  sb[i] = s;
  for (int c = 0; c < C; ++c) {
    const bool ninf = flags && ((flags[(li * rcp + r) * nw + (c >> 5)] >> (c & 31)) & 1u);
    double v = 0.0;
    if (ninf) v = -__builtin_inf();
    else if (s > 0.0) {
      const double a = ca_ll_colsum(p1 + c, n_cnt * nc1, nullptr, 0, nzc);
      const double logz = D > 0 ? ca_ll_logz(mpart + li, n_cnt, zpart + li * nc2 + (int64_t)r * C + c, n_cnt * nc2, nullptr, 0, nzc) : log(Z0[r * C + c]);
      v = a - s * logz;
    }
    llb[i * C + c] = v;
  }
}

__global__ void __launch_bounds__(CA_TB) k_boot_reduce(const double* __restrict__ llb /*[n_cnt][rc][C]*/, const double* __restrict__ lp /*[N][C], or null*/, int* __restrict__ votes,
                                                       double* __restrict__ psum, double* __restrict__ psq /*[cells of the call][C], this batch's first row*/, int64_t n_lo,
                                                       int64_t n_cnt, int rc, int C) {
#pragma clang fp contract(off)
  const int64_t li = (int64_t)blockIdx.x * CA_TB + threadIdx.x;
  if (li >= n_cnt) return;
  const double* __restrict__ pr = lp ? lp + (n_lo + li) * C : nullptr;
  for (int r = 0; r < rc; ++r) {
    const double* __restrict__ t = llb + (li * rc + r) * C;
    double m = -__builtin_inf();
    int best = 0;
    for (int c = 0; c < C; ++c) {
      const double v = t[c] + (pr ? pr[c] : 0.0);
      if (v > m) { m = v; best = c; }
    }
    votes[li * C + best] += 1;
    if (m == -__builtin_inf()) continue;   // every clone excluded: no share to add
    double z = 0.0;
    for (int c = 0; c < C; ++c) {
      const double v = t[c] + (pr ? pr[c] : 0.0);
      z += v == m ? 1.0 : exp(v - m);   // (v == m also covers m = +inf)
    }
    for (int c = 0; c < C; ++c) {
      const double v = t[c] + (pr ? pr[c] : 0.0);
      const double p = (v == m ? 1.0 : exp(v - m)) / z;
      psum[li * C + c] += p;
      psq[li * C + c] += p * p;   // (contraction is off in this kernel: the square is rounded on its own, so one call with R replicates adds what R calls with one each return)
    }
  }
}
