// ca_k_pairll.hip.h -- part of ca_kernels.hip.h (textually included there, after ca_k_loglik.hip.h): the log-likelihood of the resident counts under a MIXTURE of
// two clones (ca_clone_pair_loglik; a heterotypic doublet: the sum of two multinomial rows of clones a < b is multinomial in w p_a + (1 - w) p_b):
//   pll[n][(a,b)][w] = sum_{g: y_ng > 0} y_ng log( w E_ga / Z_na + (1 - w) E_gb / Z_nb ) + sum_g y_ng eta_ng (+ lgamma(s_n + 1) - sum_g lgamma(y_ng + 1)),
// in the notation of ca_k_loglik.hip.h.  With an exponent term (D > 0) the weight a gene sees depends on the cell through Z_na / Z_nb, so the logarithm is no
// per-gene table: it costs one float64 log per (cell, non-zero count, pair, weight).  (D = 0 IS a table -- the host builds it and k_clone_ll sweeps it.)
//
// k_pair_ll<YT>: A WAVE OWNS A CELL, THE LANES ARE THE (pair, weight) SLOTS, slot j = 64 * blockIdx.y + lane (column j = pair * W + weight of the output).
// The wave reads its row in segments of 64 * VEC columns with one coalesced 16-byte non-temporal load per lane (the next segment's in flight) and COMPACTS the
// segment's non-zero counts into a list of its own in LDS -- (gene offset, count as double), in ASCENDING gene order: one ballot per column of the lane's VEC,
// mbcnt over the lanes below, no atomic; u8 escapes (255 + an entry of the overflow list) are resolved here.  It then walks the list: the gene is wave-uniform
// (read back through readfirstlane: the row of E is a scalar base), a lane loads E[g][a] and E[g][b] of its slot from the gene's row of C doubles (one or two
// cache lines for the whole wave; the next entry's loads are issued before this entry's logarithm) and adds y log(A E_ga + B E_gb) with its slot's two coefficients, held in registers since before the first gene:
//   lz = min(log Z_na, log Z_nb),  A = w exp(lz - log Z_na),  B = (1 - w) exp(lz - log Z_nb)   (both <= 1: nothing overflows),  - s_n lz outside the sum.
// Zero counts are never listed (no 0 log 0); both E = 0 against a positive count is log 0 = -inf, which stays -inf; one E = 0 is finite.  No NaN.
// More than 64 slots are further blocks in y, each of which reads and compacts the row again (5 KB against 64 logs per non-zero count): the slot loop is
// outermost, a lane holds ONE slot, and the registers are those of one float64 log.
//
// Sums: a lane adds its slot over the cell's non-zero genes in ascending order, alone -- no cross-lane reduction, no atomic, no partial slab.  The value depends
// on the cell's row and the inputs only: not on its place in the launch, the batch or the cell range of the call; a cell-sharded group returns the single handle's bits.
//
// k_pair_cell (before it): per cell log Z_nc, merged from k_clone_ll_z's chunks by the routine k_clone_ll_finish merges them with (ca_ll_logz, ca_k_loglik.hip.h),
// and base_n = sum_g y eta (+ const) from k_clone_ll's partial sums against [log E | V] (ca_ll_yeta, ca_ll_colsum): neither is computed again here.  k_pair_ll adds base_n and subtracts s_n lz itself (the lane holds the whole sum).
// k_pair_tab_finish (D = 0): adds the segments of the table sweep's partial sums, base_n and - s_n lz of the slot.
#define CA_PLL_WMAX 8   // weights per call

__global__ void __launch_bounds__(CA_TB) k_pair_cell(const double* __restrict__ part, const double* __restrict__ lgpart /* or null */, const double* __restrict__ zpart,
                                                     const double* __restrict__ mpart, const double* __restrict__ logz0 /*[C]: D = 0*/, const double* __restrict__ Ut,
                                                     const double* __restrict__ s64, double* __restrict__ lzc /*[n_cnt][C]*/, double* __restrict__ base /*[n_cnt]*/,
                                                     int64_t n_lo, int64_t n_cnt, int C, int D, int nseg, int nct, int nzc, int nzt) {
  const int64_t i = (int64_t)blockIdx.x * CA_TB + threadIdx.x;
  if (i >= n_cnt * (C + 1)) return;
  const int64_t li = i / (C + 1);
  const int c = (int)(i - li * (C + 1));
  const int64_t n = n_lo + li;
  if (c < C) {
    lzc[li * C + c] = D > 0 ? ca_ll_logz(mpart + li, n_cnt, zpart + li * nzt + c, n_cnt * nzt, nullptr, 0, nzc) : logz0[c];
    return;
  }
  double b = D > 0 ? ca_ll_yeta(Ut + n * CA_LL_DMAX, D, part + li * nct + C, 1, n_cnt * nct, nullptr, 0, nseg) : 0.0;
  if (lgpart) b += lgamma(s64[n] + 1.0) - ca_ll_colsum(lgpart + li, n_cnt, nullptr, 0, nseg);
  base[li] = b;
}

// the clones of pair p in the lexicographic order (0,1), (0,2), ..., (C-2,C-1)
__device__ __forceinline__ void ca_pair_of(int p, int C, int& a, int& b) {
  a = 0;
  while (p >= C - 1 - a) { p -= C - 1 - a; ++a; }
  b = a + 1 + p;
}

template <typename YT>
__global__ void __launch_bounds__(CA_TB) k_pair_ll(const YT* __restrict__ Y, const double* __restrict__ Ec /*[G][C]*/, const double* __restrict__ lzc /*[n_cnt][C]*/,
                                                   const double* __restrict__ base /*[n_cnt]*/, const double* __restrict__ s64, const double* __restrict__ wts /*[W]*/,
                                                   const int64_t* __restrict__ orowptr /* or null */, const int* __restrict__ ocol, const float* __restrict__ oval,
                                                   double* __restrict__ out /*[n_cnt][MW]*/, int64_t n_lo, int64_t n_cnt, int G, int Gp, int nseg, int C, int W, int MW) {
  constexpr int VEC = YVec<YT>::VEC;
  constexpr int SEGW = 64 * VEC;   // columns per segment
  __shared__ double yv[CA_TB / 64][SEGW];
  __shared__ unsigned short gi[CA_TB / 64][SEGW];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t li = (int64_t)blockIdx.x * (CA_TB / 64) + wave;   // the wave's cell of this batch
  if (li >= n_cnt) return;   // wave-uniform (the kernel has no block barrier)
  const int64_t n = n_lo + li;
  const int j = (int)blockIdx.y * 64 + lane;   // this lane's slot
  const bool live = j < MW;
  const int jj = live ? j : MW - 1;            // (a lane past the end walks the last slot and stores nothing)
  const int pr = jj / W, wi = jj - pr * W;
  int a, b;
  ca_pair_of(pr, C, a, b);
  const double la = lzc[li * C + a], lb = lzc[li * C + b];
  const double lz = fmin(la, lb), w = wts[wi];
  const double A = w * exp(lz - la), B = (1.0 - w) * exp(lz - lb);
  long long oe0 = 0; int noe = 0;
  if constexpr (sizeof(YT) == 1) {
    if (orowptr) { oe0 = orowptr[n]; noe = (int)(orowptr[n + 1] - oe0); }   // wave-uniform
  }
  typedef unsigned v4u_ __attribute__((ext_vector_type(4)));
  const char* row = reinterpret_cast<const char*>(Y) + n * ((int64_t)Gp * (int64_t)sizeof(YT)) + lane * 16;
  double* myv = yv[wave];
  unsigned short* mgi = gi[wave];
  const double* __restrict__ ea = Ec + a;
  const double* __restrict__ eb = Ec + b;
  double acc = 0.0;
  v4u_ nxt = __builtin_nontemporal_load(reinterpret_cast<const v4u_*>(row));   // streamed once per block row
  for (int sg = 0; sg < nseg; ++sg) {
    const v4u_ cur = nxt;
    if (sg + 1 < nseg) nxt = __builtin_nontemporal_load(reinterpret_cast<const v4u_*>(row + (int64_t)(sg + 1) * SEGW * (int64_t)sizeof(YT)));
    float y[VEC];
    YVec<YT>::decode((uint4){cur.x, cur.y, cur.z, cur.w}, y);
    const int c0 = lane * VEC, g0 = sg * SEGW + c0;
    // compaction in ascending gene order: this lane's entries start behind those of the lanes below
    int below = 0, total = 0;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const unsigned long long m = __builtin_amdgcn_ballot_w64(g0 + k < G && y[k] > 0.f);
      below += (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
      total += __builtin_popcountll(m);
    }
    total = __builtin_amdgcn_readfirstlane(total);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");   // (the walk of the previous segment is done before its list is overwritten; a wave's LDS accesses stay in order)
    int pos = below;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      if (g0 + k < G && y[k] > 0.f) {
        double yd = (double)y[k];
        if constexpr (sizeof(YT) == 1) {
          if (y[k] == 255.f && noe > 0) yd += ca_mse_excess(ocol, oval, oe0, noe, g0 + k);   // rare: 255 + an entry of the overflow list
        }
        myv[pos] = yd;
        mgi[pos] = (unsigned short)(c0 + k);
        ++pos;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    const int64_t gb = (int64_t)sg * SEGW;
    // the walk, one entry ahead: the next entry's two loads of E are in flight while this entry's logarithm is taken
    double ya = 0.0, xa = 0.0, xb = 0.0;
    if (total > 0) {
      const int64_t g = gb + __builtin_amdgcn_readfirstlane((int)mgi[0]);   // wave-uniform
      ya = myv[0]; xa = ea[g * C]; xb = eb[g * C];
    }
    for (int i = 0; i < total; ++i) {
      const double yd = ya, va = xa, vb = xb;
      const int in = i + 1 < total ? i + 1 : i;   // (the last entry is loaded twice)
      const int64_t g = gb + __builtin_amdgcn_readfirstlane((int)mgi[in]);
      ya = myv[in]; xa = ea[g * C]; xb = eb[g * C];
      acc = fma(yd, log(fma(A, va, B * vb)), acc);
    }
  }
  if (live) {
    const double s = s64[n];
    double r = acc + base[li];
    if (s > 0.0) r -= s * lz;   // (a cell without counts: every term is 0)
    out[li * MW + j] = r;
  }
}

// D = 0: the slots' sums came from k_clone_ll against the table log(A P_ga + B P_gb); the segments added in ascending order, then base_n and - s_n lz of the slot
__global__ void __launch_bounds__(CA_TB) k_pair_tab_finish(const double* __restrict__ ppart /*[nseg][n_cnt][nctp]*/, const double* __restrict__ base /*[n_cnt]*/,
                                                           const double* __restrict__ slot_lz /*[MW]*/, const double* __restrict__ s64, double* __restrict__ out /*[n_cnt][MW]*/,
                                                           int64_t n_lo, int64_t n_cnt, int MW, int nseg, int nctp) {
  const int64_t i = (int64_t)blockIdx.x * CA_TB + threadIdx.x;
  if (i >= n_cnt * MW) return;
  const int64_t li = i / MW;
  const int j = (int)(i - li * MW);
  double acc = 0.0;
  for (int sg = 0; sg < nseg; ++sg) acc += ppart[((int64_t)sg * n_cnt + li) * nctp + j];
  const double s = s64[n_lo + li];
  double r = acc + base[li];
  if (s > 0.0) r -= s * slot_lz[j];
  out[li * MW + j] = r;
}
