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
#define CA_LL_PIECE 128    // bytes of a row staged per piece
#define CA_LL_PITCH 144    // bytes between rows of a staged piece
#define CA_LL_LGTAB 256    // entries of the lgamma(k + 1) table
#define CA_LL_ZCHUNK 512   // genes per block of k_clone_ll_z
#define CA_LL_DMAX 8

// lgamma(y + 1) off the table (rare): kept out of line, so that the unrolled gene loop carries one call and not sixteen copies of the routine
__device__ __noinline__ double ca_ll_lgamma1p(double y) { return lgamma(y + 1.0); }

template <typename YT, int NC>
__global__ void __launch_bounds__(CA_TB) __attribute__((amdgpu_waves_per_eu(NC <= 8 ? 4 : NC <= 16 ? 3 : 2, NC <= 8 ? 4 : NC <= 16 ? 3 : 2)))
k_clone_ll(const YT* __restrict__ Y, const double* __restrict__ tab /*[ngrp][Gp][NC]*/, const unsigned* __restrict__ zmask /*[ngrp][Gp]*/,
                                                    const double* __restrict__ lgtab /*[CA_LL_LGTAB], or null: no lgamma sum*/, const int64_t* __restrict__ orowptr /* or null */,
                                                    const int* __restrict__ ocol, const float* __restrict__ oval, double* __restrict__ part /*[nseg][n_cnt][ngrp * NC]*/,
                                                    double* __restrict__ lgpart /*[nseg][n_cnt]*/, int64_t N, int64_t n_lo, int64_t n_cnt, int G, int Gp, int nseg) {
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
  const bool lg = lgtab != nullptr && grp == 0;
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
  double lgacc = 0.0;
  const double* __restrict__ trow = tab + (int64_t)grp * Gp * NC;
  const unsigned* __restrict__ zrow = zmask + (int64_t)grp * Gp;
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
      const v4u_ t_ = *reinterpret_cast<const v4u_*>(mine + lane * CA_LL_PITCH + p * 16);
      float y[VEC];
      YVec<YT>::decode((uint4){t_.x, t_.y, t_.z, t_.w}, y);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const int g = g0 + j;
        if (g < G) {   // wave-uniform
          double yd = (double)y[j];
          if constexpr (sizeof(YT) == 1) {
            if (y[j] == 255.f && noe > 0) yd += ca_mse_excess(ocol, oval, oe0, noe, g);   // per lane, rare: 255 + an entry of the overflow list
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
          if (lg) {   // wave-uniform
            if (yd < (double)CA_LL_LGTAB && yd == (double)(int)yd) lgacc += lgt[(int)yd];
            else lgacc += ca_ll_lgamma1p(yd);
          }
        }
      }
    }
  }
  if (valid) {
    double* out = part + ((int64_t)sg * n_cnt + li) * ((int64_t)ngrp * NC) + (int64_t)grp * NC;
#pragma unroll
    for (int c = 0; c < NC; ++c) out[c] = acc[c];
    if (lg) lgpart[(int64_t)sg * n_cnt + li] = lgacc;
  }
}

template <int NC>
__global__ void __launch_bounds__(CA_TB) k_clone_ll_z(const double* __restrict__ Ut /*[N][CA_LL_DMAX], zero padded*/, const double* __restrict__ Vt /*[Gp][CA_LL_DMAX], zero padded*/,
                                                      const double* __restrict__ Ez /*[ngrp][Gp][NC]*/, double* __restrict__ zpart /*[nzc][n_cnt][ngrp * NC]*/,
                                                      double* __restrict__ mpart /*[nzc][n_cnt]*/, int64_t n_lo, int64_t n_cnt, int G, int Gp) {
  const int64_t li = (int64_t)blockIdx.x * CA_TB + threadIdx.x;
  const bool valid = li < n_cnt;
  const int64_t n = n_lo + (valid ? li : n_cnt - 1);
  const int zc = blockIdx.y, grp = blockIdx.z, ngrp = gridDim.z;
  const int g_lo = zc * CA_LL_ZCHUNK, g_hi = (g_lo + CA_LL_ZCHUNK < G) ? g_lo + CA_LL_ZCHUNK : G;   // wave-uniform
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
  double a = 0.0;
  for (int sg = 0; sg < nseg; ++sg) a += part[((int64_t)sg * n_cnt + li) * nct + c];
  double logz;
  if (D > 0) {
    double yeta = 0.0;
    for (int d = 0; d < D; ++d) {
      double yv = 0.0;
      for (int sg = 0; sg < nseg; ++sg) yv += part[((int64_t)sg * n_cnt + li) * nct + C + d];
      yeta = fma(Ut[n * CA_LL_DMAX + d], yv, yeta);
    }
    a += yeta;
    double m = -__builtin_inf();
    for (int k = 0; k < nzc; ++k) m = fmax(m, mpart[(int64_t)k * n_cnt + li]);
    double z = 0.0;
    for (int k = 0; k < nzc; ++k) z = fma(zpart[((int64_t)k * n_cnt + li) * nzt + c], exp(mpart[(int64_t)k * n_cnt + li] - m), z);
    logz = m + log(z);
  } else {
    logz = logz0[c];
  }
  const double s = s64[n];
  if (s > 0.0) a -= s * logz;   // (a cell without counts: every term is 0)
  if (lgpart) {
    double l = 0.0;
    for (int sg = 0; sg < nseg; ++sg) l += lgpart[(int64_t)sg * n_cnt + li];
    a += lgamma(s + 1.0) - l;
  }
  ll[n * C + c] = a;
}
