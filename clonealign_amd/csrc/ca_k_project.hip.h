// ca_k_project.hip.h -- part of ca_kernels.hip.h (textually included there, after ca_k_loglik.hip.h): the per-cell MAP psi and the exact clone posterior at it,
// for cells of the resident matrix under a fitted model's gene-level parameters (ca_project_cells; include/clonealign_hip.h has the algorithm):
//   maximise  F_n(psi) = logsumexp_c( ll_nc(psi) + log_prior_nc ) - |psi|^2 / 2   by generalised EM, one safeguarded Newton step per round.
// The count matrix is read ONCE, by k_clone_ll against the table [log E | V] (A = Y log E, B = Y V, the lgamma sum; ca_k_loglik.hip.h); k_proj_sums adds its
// segments (ca_ll_colsum).  A round is two launches that never read Y; eta and the merge of the chunks are ca_k_loglik.hip.h's (ca_ll_eta, ca_ll_chunk_max,
// ca_ll_chunk_sums):
//
// k_proj_mom<NC, K>: per cell and clone the exponential-family moments of W under the weights E[g][c] exp(eta_ng - m),
//   Z0 = sum_g E e,  Z1[k] = sum_g E e W[g][k],  Z2[k][l] = sum_g E e W[g][k] W[g][l] (k <= l):  NM = 1 + K + K (K + 1) / 2 sums per clone.
// k_clone_ll_z's transposed shape: A LANE OWNS A CELL and holds its U = [psi | x] in registers, a gene's rows of V and E are SCALAR operands, genes are cut
// into CA_LL_ZCHUNK-gene chunks (grid.y) so that small batches still fill the device, clones beyond NC go in further launch groups (grid.z).  Per chunk first
// the largest exponent m, then the shifted sums; ONE float64 exp per (cell, gene), shared by the NC clones and the NM moments of each (NC * NM accumulators
// per lane: 24 at K = 1, 48 at K = 2 for eight clones).  A wave whose 64 cells are all frozen returns at once.  Sums per lane in ascending gene order.
//
// k_proj_step<K>, one thread per cell: merges the chunks under the overall maximum (ascending), forms ll and the softmax over the clones (one pass with a
// running maximum, clones in ascending order), the gradient and the K x K Hessian, solves in closed form, limits the step to max_step in max-norm, and
// either freezes the cell (step <= tol BEFORE it is applied: the outputs are this round's) or moves psi.  No atomics anywhere: two calls agree bit for bit, and
// a cell's outputs depend on nothing but its own row (freezing is per cell), so a cell-sharded group returns the single handle's bits.
// Slabs: zpart[chunk][column][cell] with column = clone * NM + moment (a wave's stores and the finisher's loads are 512 contiguous bytes), mpart[chunk][cell].

#define CA_PROJ_KMAX 2   // free factors: NC * NM accumulators per lane must stay in registers (120 at K = 4 for eight clones do not)

template <int K> struct ca_proj_nm { static constexpr int value = 1 + K + K * (K + 1) / 2; };

// A[n][c] = sum over the segments of the sweep's partials (+ the multinomial constant), B[n][d] likewise: one thread per (cell, column of [log E | V])
__global__ void __launch_bounds__(CA_TB) k_proj_sums(const double* __restrict__ part /*[nseg][n_cnt][nct]*/, const double* __restrict__ lgpart /* or null */,
                                                     const double* __restrict__ s64, double* __restrict__ A /*[N][C]*/, double* __restrict__ B /*[N][CA_LL_DMAX]*/,
                                                     int64_t n_lo, int64_t n_cnt, int C, int D, int nseg, int nct) {
  const int ncol = C + D;
  const int64_t i = (int64_t)blockIdx.x * CA_TB + threadIdx.x;
  if (i >= n_cnt * ncol) return;
  const int64_t li = i / ncol;
  const int col = (int)(i - li * ncol);
  const int64_t n = n_lo + li;
  double a = ca_ll_colsum(part + li * nct + col, n_cnt * nct, nullptr, 0, nseg);
  if (col >= C) { B[n * CA_LL_DMAX + (col - C)] = a; return; }
  if (lgpart) a += lgamma(s64[n] + 1.0) - ca_ll_colsum(lgpart + li, n_cnt, nullptr, 0, nseg);
  A[n * C + col] = a;
}

template <int NC, int K>
__global__ void __launch_bounds__(CA_TB) __attribute__((amdgpu_waves_per_eu(NC * ca_proj_nm<K>::value <= 24 ? 4 : 3, NC * ca_proj_nm<K>::value <= 24 ? 4 : 3)))
k_proj_mom(const double* __restrict__ Ut /*[N][CA_LL_DMAX]: psi | x, zero padded*/, const double* __restrict__ Vt /*[Gp][CA_LL_DMAX]: W | beta, zero padded*/,
           const double* __restrict__ Ez /*[ngrp][Gp][NC]*/, const unsigned char* __restrict__ frozen /*[N]*/, double* __restrict__ zpart /*[nzc][ngrp * NC * NM][n_cnt]*/,
           double* __restrict__ mpart /*[nzc][n_cnt]*/, int64_t n_lo, int64_t n_cnt, int G, int Gp) {
  constexpr int NM = ca_proj_nm<K>::value;
  const int64_t li = (int64_t)blockIdx.x * CA_TB + threadIdx.x;
  const bool valid = li < n_cnt;
  const int64_t n = n_lo + (valid ? li : n_cnt - 1);
  const bool live = valid && frozen[n] == 0;
  if (!__any(live)) return;   // the wave's cells are all frozen (or past the end)
  const int zc = blockIdx.y, grp = blockIdx.z, ngrp = gridDim.z;
  const int g_lo = zc * CA_LL_ZCHUNK, g_hi = (g_lo + CA_LL_ZCHUNK < G) ? g_lo + CA_LL_ZCHUNK : G;   // wave-uniform
  double u[CA_LL_DMAX];
#pragma unroll
  for (int d = 0; d < CA_LL_DMAX; ++d) u[d] = Ut[n * CA_LL_DMAX + d];
  double m = -__builtin_inf();
  for (int g = g_lo; g < g_hi; ++g) m = fmax(m, ca_ll_eta(u, Vt + (int64_t)g * CA_LL_DMAX));
  double acc[NC * NM];
#pragma unroll
  for (int i = 0; i < NC * NM; ++i) acc[i] = 0.0;
  const double* __restrict__ erow = Ez + (int64_t)grp * Gp * NC;
  for (int g = g_lo; g < g_hi; ++g) {
    const double* __restrict__ v = Vt + (int64_t)g * CA_LL_DMAX;
    const double* __restrict__ er = erow + (int64_t)g * NC;
    double w[NM];   // e, e W_k, e W_k W_l (k <= l)
    w[0] = exp(ca_ll_eta(u, v) - m);
    if constexpr (K >= 1) { w[1] = w[0] * v[0]; }
    if constexpr (K == 1) { w[2] = w[1] * v[0]; }
    if constexpr (K == 2) { w[2] = w[0] * v[1]; w[3] = w[1] * v[0]; w[4] = w[1] * v[1]; w[5] = w[2] * v[1]; }
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int j = 0; j < NM; ++j) acc[c * NM + j] = fma(er[c], w[j], acc[c * NM + j]);
  }
  if (live) {
    double* out = zpart + ((int64_t)zc * ((int64_t)ngrp * NC * NM) + (int64_t)grp * NC * NM) * n_cnt + li;
#pragma unroll
    for (int i = 0; i < NC * NM; ++i) out[(int64_t)i * n_cnt] = acc[i];
    if (grp == 0) mpart[(int64_t)zc * n_cnt + li] = m;
  }
}

// One round's finisher (final = 0), or the closing evaluation of the cells that never froze (final = 1: no step, outputs at the psi they hold).
template <int K>
__global__ void __launch_bounds__(CA_TB) k_proj_step(const double* __restrict__ zpart, const double* __restrict__ mpart, const double* __restrict__ A /*[N][C]*/,
                                                     const double* __restrict__ B /*[N][CA_LL_DMAX]*/, const double* __restrict__ lp /*[N][C] or null*/,
                                                     const double* __restrict__ s64, double* __restrict__ Ut /*[N][CA_LL_DMAX]*/, unsigned char* __restrict__ frozen,
                                                     int* __restrict__ rounds, unsigned char* __restrict__ conv, double* __restrict__ ll /*[N][C]*/,
                                                     double* __restrict__ probs /*[N][C]*/, double* __restrict__ obj /*[N]*/, int64_t n_lo, int64_t n_cnt, int C,
                                                     int nzc, int nmt /* columns of a chunk's slab */, int round, int final, double tol, double max_step) {
  constexpr int NM = ca_proj_nm<K>::value;
  constexpr int NS = K * (K + 1) / 2;
  const int64_t li = (int64_t)blockIdx.x * CA_TB + threadIdx.x;
  if (li >= n_cnt) return;
  const int64_t n = n_lo + li;
  if (frozen[n]) return;
  const double m = ca_ll_chunk_max(mpart + li, n_cnt, nullptr, 0, nzc);   // (one max serves every clone of the cell)
  double ub = 0.0;
  for (int d = 0; d < CA_LL_DMAX; ++d) ub = fma(Ut[n * CA_LL_DMAX + d], B[n * CA_LL_DMAX + d], ub);
  const double s = s64[n];
  // softmax over the clones in one pass: running maximum M, sums under it of 1, mean_c and cov_c
  double M = -__builtin_inf(), S = 0.0, Sm[K > 0 ? K : 1], Sc[NS > 0 ? NS : 1];
#pragma unroll
  for (int k = 0; k < K; ++k) Sm[k] = 0.0;
#pragma unroll
  for (int k = 0; k < NS; ++k) Sc[k] = 0.0;
  for (int c = 0; c < C; ++c) {
    double z[NM];
    ca_ll_chunk_sums<NM>(m, mpart + li, n_cnt, zpart + (int64_t)c * NM * n_cnt + li, (int64_t)nmt * n_cnt, n_cnt, nullptr, 0, nzc, z);
    double a = A[n * C + c] + ub;
    if (s > 0.0) a -= s * (m + log(z[0]));   // (a cell without counts: every term is 0)
    ll[n * C + c] = a;
    const double t = lp ? a + lp[n * C + c] : a;
    if (t > -__builtin_inf()) {   // (an excluded clone weighs 0 and its moments are never formed)
      if (t > M) {
        const double r = exp(M - t);
        S *= r;
#pragma unroll
        for (int k = 0; k < K; ++k) Sm[k] *= r;
#pragma unroll
        for (int k = 0; k < NS; ++k) Sc[k] *= r;
        M = t;
      }
      const double e = exp(t - M);
      S += e;
      if constexpr (K == 1) {
        const double mu = z[1] / z[0];
        Sm[0] = fma(e, mu, Sm[0]);
        Sc[0] = fma(e, z[2] / z[0] - mu * mu, Sc[0]);
      }
      if constexpr (K == 2) {
        const double m0 = z[1] / z[0], m1 = z[2] / z[0];
        Sm[0] = fma(e, m0, Sm[0]);
        Sm[1] = fma(e, m1, Sm[1]);
        Sc[0] = fma(e, z[3] / z[0] - m0 * m0, Sc[0]);
        Sc[1] = fma(e, z[4] / z[0] - m0 * m1, Sc[1]);
        Sc[2] = fma(e, z[5] / z[0] - m1 * m1, Sc[2]);
      }
    }
  }
  const bool dead = !(M > -__builtin_inf());   // no clone is possible: the cell keeps its psi, NaN probabilities
  bool stop = final != 0 || dead;
  bool ok = final != 0 && K == 0 && !dead;
  int used = dead ? 0 : round;
  if constexpr (K > 0) {
    if (!stop) {
      double d[K], dmax;
      if constexpr (K == 1) {
        const double g0 = B[n * CA_LL_DMAX] - s * (Sm[0] / S) - Ut[n * CA_LL_DMAX];
        d[0] = g0 / (1.0 + s * (Sc[0] / S));
        dmax = fabs(d[0]);
      } else {
        const double g0 = B[n * CA_LL_DMAX] - s * (Sm[0] / S) - Ut[n * CA_LL_DMAX];
        const double g1 = B[n * CA_LL_DMAX + 1] - s * (Sm[1] / S) - Ut[n * CA_LL_DMAX + 1];
        const double h00 = 1.0 + s * (Sc[0] / S), h01 = s * (Sc[1] / S), h11 = 1.0 + s * (Sc[2] / S);
        const double det = h00 * h11 - h01 * h01;
        d[0] = (h11 * g0 - h01 * g1) / det;
        d[1] = (h00 * g1 - h01 * g0) / det;
        dmax = fmax(fabs(d[0]), fabs(d[1]));
      }
      used = round + 1;
      if (!(dmax < __builtin_inf())) stop = true;   // a step that is no number: the cell stops where it is, not converged
      else if (dmax <= tol) { stop = true; ok = true; }
      else {
        const double f = dmax > max_step ? max_step / dmax : 1.0;
#pragma unroll
        for (int k = 0; k < K; ++k) Ut[n * CA_LL_DMAX + k] += d[k] * f;
      }
    }
  }
  if (!stop) return;
  frozen[n] = 1;
  rounds[n] = used;
  conv[n] = ok ? 1 : 0;
  const double lse = M + log(S);
  double q = 0.0;
#pragma unroll
  for (int k = 0; k < K; ++k) q = fma(Ut[n * CA_LL_DMAX + k], Ut[n * CA_LL_DMAX + k], q);
  obj[n] = dead ? -__builtin_inf() : lse - 0.5 * q;
  for (int c = 0; c < C; ++c) {
    const double a = ll[n * C + c];
    const double t = lp ? a + lp[n * C + c] : a;
    probs[n * C + c] = dead ? __builtin_nan("") : exp(t - lse);
  }
}
