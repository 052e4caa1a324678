// ca_k_blockll.hip.h -- part of ca_kernels.hip.h (textually included there, after ca_k_loglik.hip.h whose constants, tables and shared pieces it uses): the sufficient
// statistics of the per-cell, per-clone log-likelihood BY BLOCK OF GENES (ca_clone_loglik_by_block).  For a labelling block_of_gene of the genes, per cell n and block b:
//   A[n][b][c] = sum_{g in b} xlogy(y_ng, E[g][c]) + sum_{g in b} y_ng eta_ng,   s[n][b] = sum_{g in b} y_ng,   lg[n][b] = sum_{g in b} lgamma(y_ng + 1),
//   logZ[n][b][c] = log sum_{g in b} E[g][c] exp(eta_ng).
// The multinomial factorises exactly over the blocks, so "what block b alone says", "how the reads are split between blocks" and "the call without block b" all
// follow from these four on the host (api.clone_loglik_by_block).
//
// k_block_ll<YT, NC> is ca_ll_walk (ca_k_loglik.hip.h: a lane owns a cell, the gene's table row is a scalar operand, rows turn the corner through the per-wave LDS
// piece, the next piece's loads in flight) with a RUN LIST (its policy RUNS = true): the host cuts the gene axis into maximal ranges of consecutive genes with one
// label and cuts them again at the segment boundaries; run r covers the genes [rcut[r], rcut[r + 1]) and a segment's runs are [rseg[sg], rseg[sg + 1]).  At a run's
// end -- a wave-uniform condition -- a lane stores its NC sums, s and lg to part[run][column][cell] (the 64 cells of a wave write 512 contiguous bytes per column)
// and clears them.  These stores are all the traffic this kernel adds to k_clone_ll.  The run-end test is taken once per 16-byte group of a row (one scalar
// compare): a group without a run end takes the walk's unrolled loop; a group that holds one takes its gene-by-gene loop, which reads its counts back from the
// staged piece (unrolling that loop, with the stores behind every gene, spilled registers in the u8 instantiations).  Both add the same terms in the same order, so
// the sums do not depend on where the run ends fall in the groups.
//
// k_block_ll_z<NC> (D > 0 only; never reads Y) is ca_ll_zchunk, the body of k_clone_ll_z, over chunks cut at label changes as well: chunk k covers the genes
// [zcut[k], zcut[k + 1]), at most CA_LL_ZCHUNK of them, all of one block.
//
// k_block_ll_finish: one thread per (cell, block, clone), the cell fastest (coalesced reads of the slabs).  Through the lists block -> runs and block -> chunks it
// adds the block's runs in ascending gene order (ca_ll_colsum), folds sum_d U[n][d] (sum_{g in b} y V_d) into A (ca_ll_yeta), merges the block's chunks of Z in
// ascending order under the block's overall max (ca_ll_logz), and writes the four outputs of the batch.  No atomics anywhere: two calls agree bit for bit, and a
// cell's values depend on nothing but its row and the labelling.
#define CA_BLL_BUDGET ((int64_t)1 << 30)   // bytes of partial slabs and batch outputs per batch of cells

template <typename YT, int NC>
__global__ void __launch_bounds__(CA_TB) __attribute__((amdgpu_waves_per_eu(NC <= 8 ? 4 : NC <= 16 ? 3 : 2, NC <= 8 ? 4 : NC <= 16 ? 3 : 2)))
k_block_ll(const YT* __restrict__ Y, const double* __restrict__ tab /*[ngrp][Gp][NC]*/, const unsigned* __restrict__ zmask /*[ngrp][Gp]*/,
           const double* __restrict__ lgtab /*[CA_LL_LGTAB], or null: no lgamma sum*/, const int64_t* __restrict__ orowptr /* or null */, const int* __restrict__ ocol,
           const float* __restrict__ oval, const int* __restrict__ rcut /*[n_runs + 2]: run r = genes [rcut[r], rcut[r + 1]); the last entry is a sentinel*/,
           const int* __restrict__ rseg /*[nseg + 1]*/, double* __restrict__ part /*[n_runs][nuse + 2][n_cnt]: the sums' columns in use, then s, then lg*/,
           int64_t N, int64_t n_lo, int64_t n_cnt, int G, int Gp, int nseg, int nuse /*table columns in use: the padding of the last group is not stored*/) {
  ca_ll_walk<YT, NC, true>(Y, tab, zmask, lgtab, orowptr, ocol, oval, n_lo, n_cnt, G, Gp, nseg, part, nullptr, rcut, rseg, nuse);
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
  double acc[NC];
  const double m = ca_ll_zchunk<NC>(Ut + n * CA_LL_DMAX, Vt, Ez + (int64_t)grp * Gp * NC, zcut[zk], zcut[zk + 1], acc);
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
  const int64_t n = n_lo + li;
  const int64_t run = (int64_t)(nct + 2) * n_cnt, chunk = (int64_t)(nzt + 1) * n_cnt;   // the slabs' strides: a run of part, a chunk of zpart
  const int q0 = brp[b], q1 = brp[b + 1];
  double a = ca_ll_colsum(part + c * n_cnt + li, run, bruns, q0, q1);
  double logz;
  if (D > 0) {
    a += ca_ll_yeta(Ut + n * CA_LL_DMAX, D, part + (int64_t)C * n_cnt + li, n_cnt, run, bruns, q0, q1);
    const int k0 = bzp[b], k1 = bzp[b + 1];
    logz = ca_ll_logz(zpart + (int64_t)nzt * n_cnt + li, chunk, zpart + c * n_cnt + li, chunk, bzk, k0, k1);
    if (k1 <= k0) logz = -__builtin_inf();   // (an empty block; a block whose E is 0 everywhere: log 0 = -inf already)
  } else {
    logz = logz0b[(int64_t)b * C + c];
  }
  A[li * ((int64_t)B * C) + j] = a;
  logZ[li * ((int64_t)B * C) + j] = logz;
  if (c == 0) {
    s[li * B + b] = ca_ll_colsum(part + (int64_t)nct * n_cnt + li, run, bruns, q0, q1);
    if (lgo) lgo[li * B + b] = ca_ll_colsum(part + (int64_t)(nct + 1) * n_cnt + li, run, bruns, q0, q1);
  }
}
