// ca_k_dmll.hip.h -- part of ca_kernels.hip.h (textually included there, after ca_k_pairll.hip.h): the DIRICHLET-MULTINOMIAL log-likelihood of the resident counts
// under every clone at a grid of concentrations (ca_clone_loglik_dm; overdispersed cell scoring).  In the notation of ca_k_loglik.hip.h, with
// p_ngc = E[g][c] exp(eta_ng) / Z_nc and a_ngc = phi_k p_ngc:
//   dm[n][c][k] = lgamma(phi_k) - lgamma(phi_k + s_n) + sum_{g: y_ng > 0} [ lgamma(y_ng + a_ngc) - lgamma(a_ngc) ] (+ lgamma(s_n + 1) - sum_g lgamma(y_ng + 1)).
// The term is not linear in y and a depends on the cell, so there is no per-gene table for any D: one float64 transcendental per (cell, non-zero count, clone,
// concentration).
//
// k_dm_ll<YT>: k_pair_ll's structure.  A WAVE OWNS A CELL, THE LANES ARE THE (clone, concentration) SLOTS, slot j = 64 * blockIdx.y + lane (column
// j = clone * K + k of the output).  The wave reads its row in segments of 64 * VEC columns with one coalesced 16-byte non-temporal load per lane (the next
// segment's in flight) and COMPACTS the segment's non-zero counts into a list of its own in LDS, in ASCENDING gene order (ballot + mbcnt, no atomic; u8 escapes
// resolved here).  A segment wider than CA_DM_LIST columns (u8: 1024) is listed and walked in parts of CA_DM_LIST columns -- the lanes of a part hold consecutive
// columns, so the order stays ascending -- which keeps the list at 9 KB per wave.  Two things differ from k_pair_ll:
//   eta at compaction time: the lane that lists an entry also computes t = exp(eta_ng - m_n), eta_ng by ca_ll_eta (ca_k_loglik.hip.h) against the padded
//     rows of Ut and Vt (the routine, hence the bits, that went into m_n = max_g eta_ng in k_clone_ll_z, so t <= 1), and stores t beside the count: one exp per non-zero count,
//     shared by all slots.  D = 0 stores 1: one route for every D.
//   the term: a = coef * E[g][c] * t with the slot's coef = phi_k exp(m_n - log Z_nc) (<= phi_k: nothing overflows), held in a register since before the first
//     gene.  For an INTEGER count y <= CA_DM_YSMALL the term is log prod_{j < y} (a + j): at most CA_DM_YSMALL factors and one log.  Otherwise (a larger
//     count or a non-integer one) it is two lgamma.  The count is wave-uniform (read back through readfirstlane), so is the branch.
//     THE BOUND: the product route is taken only while phi_max <= CA_DM_PHI_PROD = 2^100 (the host passes ysmall = 0 otherwise): a <= phi_max, so every
//     factor is below 2^100 + 8 < 2^101 and the product of 8 of them below 2^808 < DBL_MAX = 2^1024.  Downwards the product is >= a (y - 1)!: it
//     underflows only where a itself does.
// The walk is one entry ahead: the next entry's load of E is in flight during this entry's transcendental.
// Rules: zero counts are never listed; a = 0 against a positive count -- E = 0, or E > 0 with a that underflows (an extreme spread of eta, or of E) -- makes
// the entry exactly -inf (selected, never computed as inf - inf); lgamma(y + a) is finite for y > 0: no NaN.  More than 64 slots are further blocks in y.
//
// Sums: a lane adds its slot over the cell's non-zero genes in ascending order, alone -- no cross-lane reduction, no atomic, no partial slab.  The value depends
// on the cell's row and the inputs only: not on its place in the launch, the batch or the cell range of the call; a cell-sharded group returns the single handle's bits.
//
// k_dm_cell (before it): per cell log Z_nc and m_n, merged from k_clone_ll_z's chunks by ca_ll_logz (ca_k_loglik.hip.h) like every other call's (D = 0: the host's log sum_g E, m = 0),
// and per (cell, concentration) the head lgamma(phi_k) - lgamma(phi_k + s_n) + const_n, const_n from k_clone_ll's lgamma sums: none of it is computed again.
#define CA_DM_LIST 512             // entries of a wave's list in LDS (9 KB per wave: four waves per SIMD fit)
#define CA_DM_KMAX 16              // concentrations per call
#define CA_DM_YSMALL 8             // integer counts up to here take the product route
#define CA_DM_PHI_PROD 0x1p100     // ... while the largest concentration is at most this
#define CA_DM_PHI_MAX 1e300        // concentrations above are refused: lgamma(phi + s) would overflow

__global__ void __launch_bounds__(CA_TB) k_dm_cell(const double* __restrict__ lgpart /* or null */, const double* __restrict__ zpart, const double* __restrict__ mpart,
                                                   const double* __restrict__ logz0 /*[C]: D = 0*/, const double* __restrict__ s64, const double* __restrict__ conc /*[K]*/,
                                                   double* __restrict__ lzc /*[n_cnt][C]*/, double* __restrict__ mrow /*[n_cnt]*/, double* __restrict__ head /*[n_cnt][K]*/,
                                                   int64_t n_lo, int64_t n_cnt, int C, int K, int D, int nseg, int nzc, int nzt) {
  const int64_t i = (int64_t)blockIdx.x * CA_TB + threadIdx.x;
  if (i >= n_cnt * (C + K)) return;
  const int64_t li = i / (C + K);
  const int c = (int)(i - li * (C + K));
  const int64_t n = n_lo + li;
  if (c < C) {
    double logz, m = 0.0;
    if (D > 0) logz = ca_ll_logz(mpart + li, n_cnt, zpart + li * nzt + c, n_cnt * nzt, nullptr, 0, nzc, &m);
    else logz = logz0[c];
    lzc[li * C + c] = logz;
    if (c == 0) mrow[li] = m;
    return;
  }
  const int k = c - C;
  const double s = s64[n], phi = conc[k];
  double h = s > 0.0 ? lgamma(phi) - lgamma(phi + s) : 0.0;   // (a cell without counts: exactly 0)
  if (lgpart) h += lgamma(s + 1.0) - ca_ll_colsum(lgpart + li, n_cnt, nullptr, 0, nseg);
  head[li * K + k] = h;
}

// a double that is the same in every lane, as a scalar
__device__ __forceinline__ double ca_dm_uniform(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)b), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(b >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// lgamma(y + a) - lgamma(a) by two lgamma (large or non-integer counts): out of line, so that the walk carries one call and not two copies of the routine
__device__ __noinline__ double ca_dm_lgdiff(double y, double a) { return lgamma(y + a) - lgamma(a); }

template <typename YT>
__global__ void __launch_bounds__(CA_TB) __attribute__((amdgpu_waves_per_eu(4))) k_dm_ll(const YT* __restrict__ Y, const double* __restrict__ Ec /*[G][C]*/, const double* __restrict__ lzc /*[n_cnt][C]*/,
                                                 const double* __restrict__ mrow /*[n_cnt]*/, const double* __restrict__ head /*[n_cnt][K]*/,
                                                 const double* __restrict__ conc /*[K]*/, const double* __restrict__ Ut /*[N][CA_LL_DMAX], or null: D = 0*/,
                                                 const double* __restrict__ Vt /*[Gp][CA_LL_DMAX]*/, const int64_t* __restrict__ orowptr /* or null */,
                                                 const int* __restrict__ ocol, const float* __restrict__ oval, double* __restrict__ out /*[n_cnt][CK]*/, int64_t n_lo,
                                                 int64_t n_cnt, int G, int Gp, int nseg, int C, int K, int CK, int ysmall) {
  constexpr int VEC = YVec<YT>::VEC;
  constexpr int SEGW = 64 * VEC;   // columns per segment
  constexpr int LCAP = SEGW > CA_DM_LIST ? CA_DM_LIST : SEGW;   // columns listed at a time: a segment is compacted and walked in NPASS parts of LPP lanes each
  constexpr int NPASS = SEGW / LCAP, LPP = 64 / NPASS;
  __shared__ double yv[CA_TB / 64][LCAP];
  __shared__ double tv[CA_TB / 64][LCAP];
  __shared__ unsigned short gi[CA_TB / 64][LCAP];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t li = (int64_t)blockIdx.x * (CA_TB / 64) + wave;   // the wave's cell of this batch
  if (li >= n_cnt) return;   // wave-uniform (the kernel has no block barrier)
  const int64_t n = n_lo + li;
  const int j = (int)blockIdx.y * 64 + lane;   // this lane's slot
  const bool live = j < CK;
  const int jj = live ? j : CK - 1;            // (a lane past the end walks the last slot and stores nothing)
  const int c = jj / K, ki = jj - c * K;
  const double m = mrow[li];                   // wave-uniform
  const double coef = conc[ki] * exp(m - lzc[li * C + c]);
  double u[CA_LL_DMAX];                        // wave-uniform: scalar operands
#pragma unroll
  for (int d = 0; d < CA_LL_DMAX; ++d) u[d] = Ut ? Ut[n * CA_LL_DMAX + d] : 0.0;
  long long oe0 = 0; int noe = 0;
  if constexpr (sizeof(YT) == 1) {
    if (orowptr) { oe0 = orowptr[n]; noe = (int)(orowptr[n + 1] - oe0); }   // wave-uniform
  }
  typedef unsigned v4u_ __attribute__((ext_vector_type(4)));
  const char* row = reinterpret_cast<const char*>(Y) + n * ((int64_t)Gp * (int64_t)sizeof(YT)) + lane * 16;
  double* myv = yv[wave];
  double* mtv = tv[wave];
  unsigned short* mgi = gi[wave];
  const double* __restrict__ ec = Ec + c;
  const double ninf = -__builtin_inf();
  double acc = 0.0;
  v4u_ nxt = __builtin_nontemporal_load(reinterpret_cast<const v4u_*>(row));   // streamed once per block row
  v4u_ cur = nxt;
  for (int it = 0; it < nseg * NPASS; ++it) {   // one loop over the parts of all segments: one copy of the walk, and only the 16 bytes of the segment live across it
    const int sg = it / NPASS, part = it - sg * NPASS;
    if (part == 0) {
      cur = nxt;
      if (sg + 1 < nseg) nxt = __builtin_nontemporal_load(reinterpret_cast<const v4u_*>(row + (int64_t)(sg + 1) * SEGW * (int64_t)sizeof(YT)));
    }
    float y[VEC];
    YVec<YT>::decode((uint4){cur.x, cur.y, cur.z, cur.w}, y);
    const int c0 = lane * VEC, g0 = sg * SEGW + c0;
    const bool mine = NPASS == 1 || lane / LPP == part;
    // compaction in ascending gene order: this lane's entries start behind those of the lanes below (of this part: its lanes hold consecutive columns)
    int below = 0, total = 0;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const unsigned long long mk = __builtin_amdgcn_ballot_w64(mine && g0 + k < G && y[k] > 0.f);
      below += (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mk >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mk, 0u));
      total += __builtin_popcountll(mk);
    }
    total = __builtin_amdgcn_readfirstlane(total);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");   // (the walk of the previous segment is done before its list is overwritten; a wave's LDS accesses stay in order)
    int pos = below;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      if (mine && g0 + k < G && y[k] > 0.f) {
        double yd = (double)y[k];
        if constexpr (sizeof(YT) == 1) {
          if (y[k] == 255.f && noe > 0) yd += ca_mse_excess(ocol, oval, oe0, noe, g0 + k);   // rare: 255 + an entry of the overflow list
        }
        double t = 1.0;
        if (Ut) t = exp(ca_ll_eta(u, Vt + (int64_t)(g0 + k) * CA_LL_DMAX) - m);   // wave-uniform; the eta that went into m (k_clone_ll_z's: the same routine)
        myv[pos] = yd;
        mtv[pos] = t;
        mgi[pos] = (unsigned short)(c0 + k);
        ++pos;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    const int64_t gb = (int64_t)sg * SEGW;
    // the walk, one entry ahead: the next entry's load of E is in flight while this entry's transcendental is taken
    double ya = 0.0, ta = 0.0, xa = 0.0;
    if (total > 0) {
      const int64_t g = gb + __builtin_amdgcn_readfirstlane((int)mgi[0]);   // wave-uniform
      ya = myv[0]; ta = mtv[0]; xa = ec[g * C];
    }
    for (int i = 0; i < total; ++i) {
      const double yd = ca_dm_uniform(ya), a = coef * xa * ta;
      const int in = i + 1 < total ? i + 1 : i;   // (the last entry is loaded twice)
      const int64_t g = gb + __builtin_amdgcn_readfirstlane((int)mgi[in]);
      ya = myv[in]; ta = mtv[in]; xa = ec[g * C];
      double term;
      if (yd <= (double)ysmall && yd == floor(yd)) {   // wave-uniform: log prod_{j < y} (a + j)
        const int yi = (int)yd;
        double p = a;
        for (int q = 1; q < yi; ++q) p *= a + (double)q;
        term = log(p);
      } else {
        term = ca_dm_lgdiff(yd, a);
      }
      acc += a > 0.0 ? term : ninf;   // (a = 0 against a positive count: -inf, selected)
    }
  }
  if (live) out[li * CK + j] = acc + head[li * K + ki];
}
