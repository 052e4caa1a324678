// ca_k_blockll.hip.h -- part of ca_kernels.hip.h (textually included there, after ca_k_loglik.hip.h whose constants, tables and walk it shares): the sufficient
// statistics of the per-cell, per-clone log-likelihood BY BLOCK OF GENES (ca_clone_loglik_by_block).  For a labelling block_of_gene of the genes, per cell n and block b:
//   A[n][b][c] = sum_{g in b} xlogy(y_ng, E[g][c]) + sum_{g in b} y_ng eta_ng,   s[n][b] = sum_{g in b} y_ng,   lg[n][b] = sum_{g in b} lgamma(y_ng + 1),
//   logZ[n][b][c] = log sum_{g in b} E[g][c] exp(eta_ng).
// The multinomial factorises exactly over the blocks, so "what block b alone says", "how the reads are split between blocks" and "the call without block b" all
// follow from these four on the host (api.clone_loglik_by_block).
//
// k_block_ll<YT, NC> is k_clone_ll's walk (a lane owns a cell, the gene's table row is a scalar operand, rows turn the corner through the per-wave LDS piece, the
// next piece's loads in flight) with a RUN LIST: the host cuts the gene axis into maximal ranges of consecutive genes with one label and cuts them again at the
// segment boundaries; run r covers the genes [rcut[r], rcut[r + 1]) and a segment's runs are [rseg[sg], rseg[sg + 1]).  At a run's end -- a wave-uniform condition
// -- a lane stores its NC sums, s and lg to part[run][column][cell] (the 64 cells of a wave write 512 contiguous bytes per column) and clears them.  These stores
// are all the traffic this kernel adds to k_clone_ll.  The run-end test is taken once per 16-byte group of a row (one scalar compare): a group without a run end
// takes k_clone_ll's unrolled loop; a group that holds one takes a gene-by-gene loop which reads its counts back from the staged piece (unrolling that loop,
// with the stores behind every gene, spilled registers in the u8 instantiations).  Both add the same terms in the same order, so the sums do not depend on where
// the run ends fall in the groups.
//
// k_block_ll_z<NC> (D > 0 only; never reads Y) is k_clone_ll_z with its chunks cut at label changes as well: chunk k covers the genes [zcut[k], zcut[k + 1]), at most
// CA_LL_ZCHUNK of them, all of one block; per chunk the max of eta, then the sum under it.
//
// k_block_ll_finish: one thread per (cell, block, clone), the cell fastest (coalesced reads of the slabs).  It adds the block's runs in ascending gene order through
// the list block -> runs, folds sum_d U[n][d] (sum_{g in b} y V_d) into A, merges the block's chunks of Z in ascending order under the block's overall max, and
// writes the four outputs of the batch.  No atomics anywhere: two calls agree bit for bit, and a cell's values depend on nothing but its row and the labelling.
#define CA_BLL_BUDGET ((int64_t)1 << 30)   // bytes of partial slabs and batch outputs per batch of cells

template <typename YT, int NC>
__global__ void __launch_bounds__(CA_TB) __attribute__((amdgpu_waves_per_eu(NC <= 8 ? 4 : NC <= 16 ? 3 : 2, NC <= 8 ? 4 : NC <= 16 ? 3 : 2)))
k_block_ll(const YT* __restrict__ Y, const double* __restrict__ tab /*[ngrp][Gp][NC]*/, const unsigned* __restrict__ zmask /*[ngrp][Gp]*/,
           const double* __restrict__ lgtab /*[CA_LL_LGTAB], or null: no lgamma sum*/, const int64_t* __restrict__ orowptr /* or null */, const int* __restrict__ ocol,
           const float* __restrict__ oval, const int* __restrict__ rcut /*[n_runs + 2]: run r = genes [rcut[r], rcut[r + 1]); the last entry is a sentinel*/,
           const int* __restrict__ rseg /*[nseg + 1]*/, double* __restrict__ part /*[n_runs][nuse + 2][n_cnt]: the sums' columns in use, then s, then lg*/,
           int64_t N, int64_t n_lo, int64_t n_cnt, int G, int Gp, int nseg, int nuse /*table columns in use: the padding of the last group is not stored*/) {
  constexpr int VEC = YVec<YT>::VEC;
  constexpr int NP = CA_LL_PIECE / 16;                 // 16-byte loads per row of a piece
  constexpr int NLD = 64 * NP / 64;                    // load instructions per piece and wave
  constexpr int NSUB = 64 * VEC * (int)sizeof(YT) / CA_LL_PIECE;   // pieces per segment
  constexpr int SUBC = CA_LL_PIECE / (int)sizeof(YT);  // columns per piece
  __shared__ __attribute__((aligned(16))) unsigned char stage[CA_TB / 64][64 * CA_LL_PITCH];
  __shared__ double lgt[CA_LL_LGTAB];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int cb = (int)blockIdx.x / nseg;               // wave-uniform from here on
  const int sg = (int)blockIdx.x - cb * nseg;
  const int grp = blockIdx.y;
  const bool first = grp == 0;                         // the group that also carries s and lg
  const bool lg = lgtab != nullptr && first;
  if (lg) {
    for (int i = threadIdx.x; i < CA_LL_LGTAB; i += CA_TB) lgt[i] = lgtab[i];
    __syncthreads();
  }
  const int64_t l0 = (int64_t)cb * CA_TB + wave * 64;  // the wave's first cell of this batch
  const int64_t li = l0 + lane;                        // this lane's cell (local)
  const bool valid = li < n_cnt;
  const int64_t n = n_lo + (valid ? li : n_cnt - 1);   // (a lane past the end walks the last cell and stores nothing)
  const int64_t pitch = (int64_t)Gp * (int64_t)sizeof(YT);
  const int lrow = lane / NP, lpc = lane % NP;
  const char* src[NLD];
#pragma unroll
  for (int i = 0; i < NLD; ++i) {
    int64_t r = l0 + i * (64 / NP) + lrow;
    if (r >= n_cnt) r = n_cnt - 1;
    src[i] = reinterpret_cast<const char*>(Y) + (n_lo + r) * pitch + (int64_t)sg * 64 * VEC * (int64_t)sizeof(YT) + lpc * 16;
  }
  typedef unsigned v4u_ __attribute__((ext_vector_type(4)));
  v4u_ nxt[NLD];
  auto fetch = [&](int sub) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) nxt[i] = __builtin_nontemporal_load(reinterpret_cast<const v4u_*>(src[i] + sub * CA_LL_PIECE));   // streamed once
  };
  unsigned char* mine = stage[wave];
  long long oe0 = 0; int noe = 0;
  if constexpr (sizeof(YT) == 1) {
    if (orowptr) { oe0 = orowptr[n]; noe = (int)(orowptr[n + 1] - oe0); }
  }
  double acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = 0.0;
  double sacc = 0.0, lgacc = 0.0;
  const double* __restrict__ trow = tab + (int64_t)grp * Gp * NC;
  const unsigned* __restrict__ zrow = zmask + (int64_t)grp * Gp;
  const int64_t ncol = nuse + 2;
  int run = rseg[sg];                                  // the current run and one past its last gene: scalars
  int nend = rcut[run + 1];
  // one gene of this lane's cell
  auto step = [&](float yf, int g) {
    double yd = (double)yf;
    if constexpr (sizeof(YT) == 1) {
      if (yf == 255.f && noe > 0) yd += ca_mse_excess(ocol, oval, oe0, noe, g);   // per lane, rare: 255 + an entry of the overflow list
    }
    const double* __restrict__ tr = trow + (int64_t)g * NC;
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = fma(yd, tr[c], acc[c]);
    const unsigned zm = zrow[g];
    if (zm != 0u) {   // wave-uniform, rare: columns of this gene with E = 0 (their table entry is 0)
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (((zm >> c) & 1u) && yd > 0.0) acc[c] = -__builtin_inf();
    }
    if (first) {   // wave-uniform
      sacc += yd;
      if (lg) {
        if (yd < (double)CA_LL_LGTAB && yd == (double)(int)yd) lgacc += lgt[(int)yd];
        else lgacc += ca_ll_lgamma1p(yd);
      }
    }
  };
  // the end of a run: its sums to the slab, coalesced over the wave's cells, and the next run begins at 0
  auto flush = [&]() {
    if (valid) {
      double* out = part + ((int64_t)run * ncol + (int64_t)grp * NC) * n_cnt + li;
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (grp * NC + c < nuse) out[(int64_t)c * n_cnt] = acc[c];   // scalar
      if (first) {
        double* sl = part + ((int64_t)run * ncol + nuse) * n_cnt + li;
        sl[0] = sacc;
        if (lg) sl[n_cnt] = lgacc;
      }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = 0.0;
    sacc = 0.0; lgacc = 0.0;
    ++run;
    nend = rcut[run + 1];
  };
  fetch(0);
  for (int sub = 0; sub < NSUB; ++sub) {
    const int gb = sg * 64 * VEC + sub * SUBC;
    if (gb >= G) break;   // (padding columns only from here on)
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");   // (the reads of the previous piece are done before it is overwritten; a wave's LDS accesses stay in order)
#pragma unroll
    for (int i = 0; i < NLD; ++i)
      *reinterpret_cast<v4u_*>(mine + (i * (64 / NP) + lrow) * CA_LL_PITCH + lpc * 16) = nxt[i];
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    if (sub + 1 < NSUB && gb + SUBC < G) fetch(sub + 1);
    for (int p = 0; p < NP; ++p) {
      const int g0 = gb + p * VEC;
      if (g0 >= G) break;
      if (nend > g0 + VEC) {   // scalar: no run ends in this group (so all its genes are below G)
        const v4u_ t_ = *reinterpret_cast<const v4u_*>(mine + lane * CA_LL_PITCH + p * 16);
        float y[VEC];
        YVec<YT>::decode((uint4){t_.x, t_.y, t_.z, t_.w}, y);
#pragma unroll
        for (int j = 0; j < VEC; ++j) step(y[j], g0 + j);
      } else {                 // a run ends here (the last gene of a segment and gene G - 1 always end one): gene by gene, the counts read back from the staged piece
#pragma unroll 1
        for (int j = 0; j < VEC; ++j) {
          const int g = g0 + j;
          if (g >= G) break;
          step((float)*reinterpret_cast<const YT*>(mine + lane * CA_LL_PITCH + p * 16 + j * (int)sizeof(YT)), g);
          if (g + 1 == nend) flush();   // scalar
        }
      }
    }
  }
}

template <int NC>
__global__ void __launch_bounds__(CA_TB) k_block_ll_z(const double* __restrict__ Ut /*[N][CA_LL_DMAX], zero padded*/, const double* __restrict__ Vt /*[Gp][CA_LL_DMAX], zero padded*/,
                                                      const double* __restrict__ Ez /*[ngrp][Gp][NC]*/, const int* __restrict__ zcut /*[nzk + 1]: chunk k = genes [zcut[k], zcut[k + 1])*/,
                                                      double* __restrict__ zpart /*[nzk][C + 1][n_cnt]: the clones' sums, then the chunk's max of eta*/,
                                                      int64_t n_lo, int64_t n_cnt, int Gp, int nzk, int C) {
  const int cb = (int)(blockIdx.x / (unsigned)nzk), zk = (int)(blockIdx.x - (unsigned)cb * (unsigned)nzk);   // wave-uniform
  const int64_t li = (int64_t)cb * CA_TB + threadIdx.x;
  const bool valid = li < n_cnt;
  const int64_t n = n_lo + (valid ? li : n_cnt - 1);
  const int grp = blockIdx.y;
  const int g_lo = zcut[zk], g_hi = zcut[zk + 1];
  double u[CA_LL_DMAX];
#pragma unroll
  for (int d = 0; d < CA_LL_DMAX; ++d) u[d] = Ut[n * CA_LL_DMAX + d];
  auto eta_of = [&](int g) {
    const double* __restrict__ v = Vt + (int64_t)g * CA_LL_DMAX;
    double e = 0.0;
#pragma unroll
    for (int d = 0; d < CA_LL_DMAX; ++d) e = fma(u[d], v[d], e);
    return e;
  };
  double m = -__builtin_inf();
  for (int g = g_lo; g < g_hi; ++g) m = fmax(m, eta_of(g));
  double acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = 0.0;
  const double* __restrict__ erow = Ez + (int64_t)grp * Gp * NC;
  for (int g = g_lo; g < g_hi; ++g) {
    const double w = exp(eta_of(g) - m);
    const double* __restrict__ er = erow + (int64_t)g * NC;
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = fma(er[c], w, acc[c]);
  }
  if (valid) {
    double* out = zpart + ((int64_t)zk * (C + 1) + (int64_t)grp * NC) * n_cnt + li;
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (grp * NC + c < C) out[(int64_t)c * n_cnt] = acc[c];   // scalar: the padding of the last group is not stored
    if (grp == 0) zpart[((int64_t)zk * (C + 1) + C) * n_cnt + li] = m;
  }
}

// the batch's four outputs from the slabs: one thread per (cell, block, clone), the cell fastest
__global__ void __launch_bounds__(CA_TB) k_block_ll_finish(const double* __restrict__ part /*[n_runs][C + D + 2][n_cnt]*/, const double* __restrict__ zpart /*[nzk][C + 1][n_cnt]*/,
                                                           const double* __restrict__ logz0b /*[B][C]: D = 0*/, const double* __restrict__ Ut,
                                                           const int* __restrict__ brp /*[B + 1]*/, const int* __restrict__ bruns, const int* __restrict__ bzp /*[B + 1]*/,
                                                           const int* __restrict__ bzk, double* __restrict__ A /*[n_cnt][B C]*/, double* __restrict__ logZ /*[n_cnt][B C]*/,
                                                           double* __restrict__ s /*[n_cnt][B]*/, double* __restrict__ lgo /*[n_cnt][B], or null*/, int64_t n_lo, int64_t n_cnt,
                                                           int B, int C, int D) {
  const int64_t i = (int64_t)blockIdx.x * CA_TB + threadIdx.x;
  if (i >= n_cnt * B * C) return;
  const int64_t j = i / n_cnt, li = i - j * n_cnt;
  const int b = (int)(j / C), c = (int)(j - (int64_t)b * C);
  const int nct = C + D, nzt = C;                      // columns in use of the two slabs
  const int64_t n = n_lo + li, ncol = nct + 2;
  const int q0 = brp[b], q1 = brp[b + 1];
  double a = 0.0;
  for (int q = q0; q < q1; ++q) a += part[((int64_t)bruns[q] * ncol + c) * n_cnt + li];
  double logz;
  if (D > 0) {
    double yeta = 0.0;
    for (int d = 0; d < D; ++d) {
      double yv = 0.0;
      for (int q = q0; q < q1; ++q) yv += part[((int64_t)bruns[q] * ncol + C + d) * n_cnt + li];
      yeta = fma(Ut[n * CA_LL_DMAX + d], yv, yeta);
    }
    a += yeta;
    const int k0 = bzp[b], k1 = bzp[b + 1];
    double m = -__builtin_inf();
    for (int k = k0; k < k1; ++k) m = fmax(m, zpart[((int64_t)bzk[k] * (nzt + 1) + nzt) * n_cnt + li]);
    double z = 0.0;
    for (int k = k0; k < k1; ++k) {
      const int64_t base = (int64_t)bzk[k] * (nzt + 1);
      z = fma(zpart[(base + c) * n_cnt + li], exp(zpart[(base + nzt) * n_cnt + li] - m), z);
    }
    logz = k1 > k0 ? m + log(z) : -__builtin_inf();   // (an empty block; a block whose E is 0 everywhere: log 0 = -inf)
  } else {
    logz = logz0b[(int64_t)b * C + c];
  }
  A[li * ((int64_t)B * C) + j] = a;
  logZ[li * ((int64_t)B * C) + j] = logz;
  if (c == 0) {
    double sv = 0.0;
    for (int q = q0; q < q1; ++q) sv += part[((int64_t)bruns[q] * ncol + nct) * n_cnt + li];
    s[li * B + b] = sv;
    if (lgo) {
      double l = 0.0;
      for (int q = q0; q < q1; ++q) l += part[((int64_t)bruns[q] * ncol + nct + 1) * n_cnt + li];
      lgo[li * B + b] = l;
    }
  }
}
