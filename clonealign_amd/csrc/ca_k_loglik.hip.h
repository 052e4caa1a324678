// ca_k_loglik.hip.h -- part of ca_kernels.hip.h (textually included there, in this order): the per-cell, per-clone log-likelihood of the resident count matrix
// under a fitted model at its point estimates (ca_clone_loglik; p_y_on_c of R/inference-tflow.R:288-296 with mu_samples replaced by the point estimate):
//   ll[n][c] = sum_g xlogy(y_ng, E[g][c]) + sum_g y_ng eta_ng - s_n log sum_g E[g][c] exp(eta_ng) (+ lgamma(s_n + 1) - sum_g lgamma(y_ng + 1)),  eta = U V^T.
//
// k_clone_ll<YT, NC>: one sweep over the [N][Gp] matrix in its own storage (u8 + overflow list, u16, f32), everything in float64.  Against a table of NC
// columns per gene -- log E of the clones, then the D columns of V, zero padded -- every cell needs NC sums over the genes, so the walk is k_fit_mse's
// TRANSPOSED: a LANE OWNS A CELL.  The gene is then wave-uniform, the table row of a gene is a scalar operand (one 8 * NC-byte scalar load per gene and wave, no
// LDS or vector register traffic per multiply-add), the NC sums of a cell stay in its lane's registers from the first gene of the segment to the last, and
// no cross-lane reduction exists at all.  Rows still come from memory as in k_fit_mse -- a wave reads 128 contiguous bytes of eight rows per 16-byte
// non-temporal load -- and turn the corner through LDS: each wave stages a 64-row x 128-byte piece of its own (rows padded to 144 bytes: conflict-free
// 16-byte reads down a column of rows), with the next piece's loads in flight in registers while the current one is consumed.
//
// Zero counts are not skipped: with a lane per cell a wave could skip a gene only where all its 64 cells hold a zero (0.8^64 at 80 % zeros).  xlogy: the
// table holds 0 where E = 0 and a bit mask of those columns per gene (zmask, wave-uniform and almost always 0); a positive count against such a column
// sets that sum to -inf, a zero count adds 0 -- no 0 * inf is ever formed, so no NaN.
// lgamma(y + 1): looked up in a 256-entry table in LDS for integer counts below 256, evaluated directly otherwise (escaped u8 counts, large u16 counts,
// non-integer f32 values); entry 0 is exactly 0.
//
// Sums, all in a fixed order (no atomics; two calls agree bit for bit): a lane adds its cell's genes of one segment in ascending order -> part[segment][cell][column]
// -> k_clone_ll_finish adds the segments ascending.  A cell's sums depend on nothing but its row, so a cell-sharded group returns the single handle's bits.
//
// k_clone_ll_z<NC> (D > 0 only; never reads Y): Z[n][c] = sum_g E[g][c] exp(eta_ng - m), again a lane per cell with V's and E's rows as scalar operands, per
// chunk of CA_LL_ZCHUNK genes: first the chunk's max of eta (m), then the sum; the finishing kernel merges the chunks in ascending order under the overall max.
//
// This file also holds what the other scoring kernels (ca_k_blockll / pairll / dmll / project / evidence.hip.h) share with these: eta (ca_ll_eta), the chunk of
// the contraction (ca_ll_zchunk), the merge of the chunks (ca_ll_merge, ca_ll_logz), the sums over the sweep's slab (ca_ll_colsum, ca_ll_yeta) and the walk
// itself (ca_ll_walk).  k_clone_ll, k_clone_ll_z and k_clone_ll_finish below are thin kernels over them.
#define CA_LL_PIECE 128    // bytes of a row staged per piece
#define CA_LL_PITCH 144    // bytes between rows of a staged piece
#define CA_LL_LGTAB 256    // entries of the lgamma(k + 1) table
#define CA_LL_ZCHUNK 512   // genes per block of k_clone_ll_z
#define CA_LL_DMAX 8

// lgamma(y + 1) off the table (rare): kept out of line, so that the unrolled gene loop carries one call and not sixteen copies of the routine
__device__ __noinline__ double ca_ll_lgamma1p(double y) { return lgamma(y + 1.0); }

// ---- the pieces the scoring kernels share (ca_k_blockll / pairll / dmll / project / evidence.hip.h call into them: one copy of the arithmetic, so the
// ---- calls return each other's bits by construction)

// eta_ng = sum_d U[n][d] V[g][d] over the CA_LL_DMAX padded factors, d ascending: one chain of fmas from 0
__device__ __forceinline__ double ca_ll_eta(const double (&u)[CA_LL_DMAX], const double* __restrict__ v /*[CA_LL_DMAX]*/) {
  double e = 0.0;
#pragma unroll
  for (int d = 0; d < CA_LL_DMAX; ++d) e = fma(u[d], v[d], e);
  return e;
}

// One chunk [g_lo, g_hi) of the contraction for a lane's cell: the max m of eta over the chunk, then acc[c] = sum_g E[g][c] exp(eta_ng - m), g ascending.
// A gene's rows of V and E are scalar operands (the bounds are wave-uniform).  Returns m.
template <int NC>
__device__ __forceinline__ double ca_ll_zchunk(const double* __restrict__ Un /*[CA_LL_DMAX]: the cell's row of Ut*/, const double* __restrict__ Vt, const double* __restrict__ erow /*[Gp][NC]*/,
                                               int g_lo, int g_hi, double (&acc)[NC]) {
  double u[CA_LL_DMAX];
#pragma unroll
  for (int d = 0; d < CA_LL_DMAX; ++d) u[d] = Un[d];
  double m = -__builtin_inf();
  for (int g = g_lo; g < g_hi; ++g) m = fmax(m, ca_ll_eta(u, Vt + (int64_t)g * CA_LL_DMAX));
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = 0.0;
  for (int g = g_lo; g < g_hi; ++g) {
    const double w = exp(ca_ll_eta(u, Vt + (int64_t)g * CA_LL_DMAX) - m);
    const double* __restrict__ er = erow + (int64_t)g * NC;
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = fma(er[c], w, acc[c]);
  }
  return m;
}

// The chunks' partial sums merged under their overall max, k ascending in [k0, k1): m = max_k m_k, then z[j] = sum_k zpart_kj exp(m_k - m), one fma per term.
// Addressing by the slab's strides: chunk k's max is mp[ck * ms] and its sum of moment j zp[ck * zs + j * zj], with ck = list ? list[k] : k (k_block_ll_finish
// goes through its list block -> chunks).  NM = 1 is the scalar case, log Z = m + log z (ca_ll_logz); the Newton rounds merge all their moments at once.
__device__ __forceinline__ double ca_ll_chunk_max(const double* __restrict__ mp, int64_t ms, const int* __restrict__ list, int k0, int k1) {
  double m = -__builtin_inf();
  for (int k = k0; k < k1; ++k) m = fmax(m, mp[(int64_t)(list ? list[k] : k) * ms]);
  return m;
}
template <int NM>
__device__ __forceinline__ void ca_ll_chunk_sums(double m, const double* __restrict__ mp, int64_t ms, const double* __restrict__ zp, int64_t zs, int64_t zj, const int* __restrict__ list,
                                                 int k0, int k1, double (&z)[NM]) {
#pragma unroll
  for (int j = 0; j < NM; ++j) z[j] = 0.0;
  for (int k = k0; k < k1; ++k) {
    const int64_t ck = list ? list[k] : k;
    const double wk = exp(mp[ck * ms] - m);
#pragma unroll
    for (int j = 0; j < NM; ++j) z[j] = fma(zp[ck * zs + j * zj], wk, z[j]);
  }
}
template <int NM>
__device__ __forceinline__ double ca_ll_merge(const double* __restrict__ mp, int64_t ms, const double* __restrict__ zp, int64_t zs, int64_t zj, const int* __restrict__ list, int k0, int k1,
                                              double (&z)[NM]) {
  const double m = ca_ll_chunk_max(mp, ms, list, k0, k1);
  ca_ll_chunk_sums<NM>(m, mp, ms, zp, zs, zj, list, k0, k1, z);
  return m;
}
__device__ __forceinline__ double ca_ll_logz(const double* __restrict__ mp, int64_t ms, const double* __restrict__ zp, int64_t zs, const int* __restrict__ list, int k0, int k1, double* m_out = nullptr) {
  double z[1];
  const double m = ca_ll_merge<1>(mp, ms, zp, zs, 0, list, k0, k1, z);
  if (m_out) *m_out = m;
  return m + log(z[0]);
}

// One column of a cell summed over the sweep's slab entries q in [q0, q1), ascending from 0: p[(list ? list[q] : q) * stride] (the segments of k_clone_ll's slab,
// or a block's runs of k_block_ll's through the list block -> runs)
__device__ __forceinline__ double ca_ll_colsum(const double* __restrict__ p, int64_t stride, const int* __restrict__ list, int q0, int q1) {
  double a = 0.0;
  for (int q = q0; q < q1; ++q) a += p[(int64_t)(list ? list[q] : q) * stride];
  return a;
}
// sum_g y_ng eta_ng of a cell from the sweep's V columns: sum_d U[n][d] * (column d of V summed as above), d ascending, one fma per factor; pv is the cell's
// first V column in entry 0, the columns dstride apart
__device__ __forceinline__ double ca_ll_yeta(const double* __restrict__ Un, int D, const double* __restrict__ pv, int64_t dstride, int64_t stride, const int* __restrict__ list, int q0, int q1) {
  double yeta = 0.0;
  for (int d = 0; d < D; ++d) yeta = fma(Un[d], ca_ll_colsum(pv + d * dstride, stride, list, q0, q1), yeta);
  return yeta;
}

// ---- the walk in which a lane owns a cell (k_clone_ll, k_block_ll): the staging constants, the loads' addresses, the stage-and-fence piece loop, the overflow
// ---- lookup and the per-gene update (the fma over NC, the zero mask, s, the lgamma table) are here once.  Where the sums go is the compile-time policy RUNS:
// ----   false (k_clone_ll): one set of sums per segment, stored after its last gene -- the instantiation carries no run-list register and no gene-by-gene loop;
// ----   true (k_block_ll): a run list cuts the segment (ca_k_blockll.hip.h has the rules): the sums, s and lg are stored and cleared wherever a run ends.
// ---- The outputs and the run list are __restrict__ PARAMETERS, not members of a policy object: through an object the compiler no longer proved that the
// ---- stores at the run ends leave the table alone, loaded the table rows into vector registers (2 NC more of them) and spilled.
template <typename YT, int NC, bool RUNS>
__device__ __forceinline__ void ca_ll_walk(const YT* __restrict__ Y, const double* __restrict__ tab /*[ngrp][Gp][NC]*/, const unsigned* __restrict__ zmask /*[ngrp][Gp]*/,
                                           const double* __restrict__ lgtab /*[CA_LL_LGTAB], or null: no lgamma sum*/, const int64_t* __restrict__ orowptr /* or null */,
                                           const int* __restrict__ ocol, const float* __restrict__ oval, int64_t n_lo, int64_t n_cnt, int G, int Gp, int nseg,
                                           double* __restrict__ part /*segments: [nseg][n_cnt][ngrp * NC]; runs: [n_runs][nuse + 2][n_cnt], the sums' columns in use, then s, then lg*/,
                                           double* __restrict__ lgpart /*segments: [nseg][n_cnt]*/, const int* __restrict__ rcut /*runs: [n_runs + 2]*/,
                                           const int* __restrict__ rseg /*runs: [nseg + 1]*/, int nuse /*runs: table columns in use*/) {
  constexpr int VEC = YVec<YT>::VEC;
  constexpr int NP = CA_LL_PIECE / 16;                 // 16-byte loads per row of a piece
  constexpr int NLD = 64 * NP / 64;                    // load instructions per piece and wave (64 rows x NP loads over 64 lanes)
  constexpr int NSUB = 64 * VEC * (int)sizeof(YT) / CA_LL_PIECE;   // pieces per segment
  constexpr int SUBC = CA_LL_PIECE / (int)sizeof(YT);  // columns per piece
  __shared__ __attribute__((aligned(16))) unsigned char stage[CA_TB / 64][64 * CA_LL_PITCH];
  __shared__ double lgt[CA_LL_LGTAB];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int cb = (int)blockIdx.x / nseg;               // wave-uniform from here on
  const int sg = (int)blockIdx.x - cb * nseg;
  const int grp = blockIdx.y, ngrp = gridDim.y;
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
  // loads: instruction i of a piece takes rows 8 i .. 8 i + 7, 128 contiguous bytes of each
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
  int run = 0, nend = 0;                               // with a run list: the current run and one past its last gene (scalars)
  if constexpr (RUNS) { run = rseg[sg]; nend = rcut[run + 1]; }
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
    if (RUNS ? first : lg) {   // wave-uniform: the group that carries s (with a run list) and lg
      if (RUNS) sacc += yd;
      if (lg) {
        if (yd < (double)CA_LL_LGTAB && yd == (double)(int)yd) lgacc += lgt[(int)yd];
        else lgacc += ca_ll_lgamma1p(yd);
      }
    }
  };
  // the end of a run: its sums to the slab, coalesced over the wave's cells, and the next run begins at 0
  auto flush = [&]() {
    if constexpr (RUNS) {
      const int64_t ncol = nuse + 2;
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
    }
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
      if (!RUNS || nend > g0 + VEC) {   // scalar: no run ends in this 16-byte group (with a run list: so all its genes are below G)
        const v4u_ t_ = *reinterpret_cast<const v4u_*>(mine + lane * CA_LL_PITCH + p * 16);
        float y[VEC];
        YVec<YT>::decode((uint4){t_.x, t_.y, t_.z, t_.w}, y);
#pragma unroll
        for (int j = 0; j < VEC; ++j)
          if (RUNS || g0 + j < G) step(y[j], g0 + j);   // wave-uniform
      } else if constexpr (RUNS) {   // a run ends here (the last gene of a segment and gene G - 1 always end one): gene by gene, the counts read back from the staged piece
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
  if constexpr (!RUNS) {   // the segment's sums
    if (valid) {
      double* out = part + ((int64_t)sg * n_cnt + li) * ((int64_t)ngrp * NC) + (int64_t)grp * NC;
#pragma unroll
      for (int c = 0; c < NC; ++c) out[c] = acc[c];
      if (lg) lgpart[(int64_t)sg * n_cnt + li] = lgacc;
    }
  }
}

// the sweep of ca_clone_loglik: the walk, a lane's NC sums (and the lgamma sum) of its segment stored at the end
template <typename YT, int NC>
__global__ void __launch_bounds__(CA_TB) __attribute__((amdgpu_waves_per_eu(NC <= 8 ? 4 : NC <= 16 ? 3 : 2, NC <= 8 ? 4 : NC <= 16 ? 3 : 2)))
k_clone_ll(const YT* __restrict__ Y, const double* __restrict__ tab /*[ngrp][Gp][NC]*/, const unsigned* __restrict__ zmask /*[ngrp][Gp]*/,
                                                    const double* __restrict__ lgtab /*[CA_LL_LGTAB], or null: no lgamma sum*/, const int64_t* __restrict__ orowptr /* or null */,
                                                    const int* __restrict__ ocol, const float* __restrict__ oval, double* __restrict__ part /*[nseg][n_cnt][ngrp * NC]*/,
                                                    double* __restrict__ lgpart /*[nseg][n_cnt]*/, int64_t N, int64_t n_lo, int64_t n_cnt, int G, int Gp, int nseg) {
  ca_ll_walk<YT, NC, false>(Y, tab, zmask, lgtab, orowptr, ocol, oval, n_lo, n_cnt, G, Gp, nseg, part, lgpart, nullptr, nullptr, 0);
}

// the contraction of ca_clone_loglik (D > 0): chunk zc = genes [zc CA_LL_ZCHUNK, (zc + 1) CA_LL_ZCHUNK), the sums to zpart[chunk][cell][column], the max to mpart[chunk][cell]
template <int NC>
__global__ void __launch_bounds__(CA_TB) k_clone_ll_z(const double* __restrict__ Ut /*[N][CA_LL_DMAX], zero padded*/, const double* __restrict__ Vt /*[Gp][CA_LL_DMAX], zero padded*/,
                                                      const double* __restrict__ Ez /*[ngrp][Gp][NC]*/, double* __restrict__ zpart /*[nzc][n_cnt][ngrp * NC]*/,
                                                      double* __restrict__ mpart /*[nzc][n_cnt]*/, int64_t n_lo, int64_t n_cnt, int G, int Gp) {
  const int64_t li = (int64_t)blockIdx.x * CA_TB + threadIdx.x;
  const bool valid = li < n_cnt;
  const int64_t n = n_lo + (valid ? li : n_cnt - 1);
  const int zc = blockIdx.y, grp = blockIdx.z, ngrp = gridDim.z;
  const int g_lo = zc * CA_LL_ZCHUNK, g_hi = (g_lo + CA_LL_ZCHUNK < G) ? g_lo + CA_LL_ZCHUNK : G;   // wave-uniform
  double acc[NC];
  const double m = ca_ll_zchunk<NC>(Ut + n * CA_LL_DMAX, Vt, Ez + (int64_t)grp * Gp * NC, g_lo, g_hi, acc);
  if (valid) {
    double* out = zpart + ((int64_t)zc * n_cnt + li) * ((int64_t)ngrp * NC) + (int64_t)grp * NC;
#pragma unroll
    for (int c = 0; c < NC; ++c) out[c] = acc[c];
    if (grp == 0) mpart[(int64_t)zc * n_cnt + li] = m;
  }
}

// ll[n][c] from the sums: the segments (and the chunks of Z under their overall max) added in ascending order; one thread per (cell, clone), row-major [N][C]
__global__ void __launch_bounds__(CA_TB) k_clone_ll_finish(const double* __restrict__ part, const double* __restrict__ lgpart /* or null */, const double* __restrict__ zpart,
                                                           const double* __restrict__ mpart, const double* __restrict__ logz0 /*[C]: D = 0*/,
                                                           const double* __restrict__ Ut, const double* __restrict__ s64, double* __restrict__ ll /*[N][C]*/,
                                                           int64_t n_lo, int64_t n_cnt, int C, int D, int nseg, int nct, int nzc, int nzt) {
  const int64_t i = (int64_t)blockIdx.x * CA_TB + threadIdx.x;
  if (i >= n_cnt * C) return;
  const int64_t li = i / C;
  const int c = (int)(i - li * C);
  const int64_t n = n_lo + li;
  const int64_t seg = n_cnt * nct;                     // the slabs' strides: a segment of part, a chunk of zpart
  double a = ca_ll_colsum(part + li * nct + c, seg, nullptr, 0, nseg);
  double logz;
  if (D > 0) {
    a += ca_ll_yeta(Ut + n * CA_LL_DMAX, D, part + li * nct + C, 1, seg, nullptr, 0, nseg);
    logz = ca_ll_logz(mpart + li, n_cnt, zpart + li * nzt + c, n_cnt * nzt, nullptr, 0, nzc);
  } else {
    logz = logz0[c];
  }
  const double s = s64[n];
  if (s > 0.0) a -= s * logz;   // (a cell without counts: every term is 0)
  if (lgpart) a += lgamma(s + 1.0) - ca_ll_colsum(lgpart + li, n_cnt, nullptr, 0, nseg);
  ll[n * C + c] = a;
}
