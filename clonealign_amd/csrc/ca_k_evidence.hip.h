// ca_k_evidence.hip.h -- part of ca_kernels.hip.h (textually included there, after ca_k_project.hip.h): the clone evidence with psi integrated out,
//   log p(y_n | c) = log Integral Normal(psi; 0, I_K) Multinomial(y_n | p_n.c(psi)) dpsi        (ca_clone_evidence; include/clonealign_hip.h has the algorithm),
// per (cell, clone): the mode of f_nc(psi) = A_nc + psi . B_n[:K] + x_n . B_n[K:] - s_n log Z_c(psi, x_n) - |psi|^2 / 2 by safeguarded Newton, the Laplace value
// f(psi*) - 1/2 log det H, and a quadrature of exp(f - f(psi*)) at the caller's nodes, centred at the mode and scaled by the Cholesky factor of H.
// The count matrix is read ONCE, by k_clone_ll and k_proj_sums (A, B, s, the lgamma constant; ca_k_loglik.hip.h, ca_k_project.hip.h).  Nothing here reads it.
//
// k_ev_mom<NS, K, FULL>: k_proj_mom's shape -- A LANE OWNS A CELL, a gene's rows of V and E are SCALAR operands, genes in CA_LL_ZCHUNK-gene chunks (grid.y) --
//   but psi is PER SLOT: a slot is a clone in the Newton rounds (FULL: all NM = 1 + K + K (K + 1) / 2 moments) and a (clone, node) in the quadrature pass
//   (Z0 only).  The x . beta_g part of the exponent is formed once per (cell, gene) and shared by the NS slots of the group (grid.z); the exp is per (cell,
//   gene, slot).  Per chunk first the largest exponent of every slot, then the shifted sums in ascending gene order.  A wave none of whose pairs is live
//   (Newton: not frozen; quadrature: possible) returns at once.
// k_ev_init: one thread per (cell, clone): psi = start; a pair with A = -inf is DEAD (evidence = laplace = -inf, rounds 0, converged 0, precision I).
// k_ev_step<K>: one thread per (cell, clone): merges the chunks under the pair's overall maximum (ascending; ca_ll_merge of ca_k_loglik.hip.h with all moments,
//   k_ev_reduce with one), f, the gradient and the K x K Hessian, the
//   closed-form solve, the step limited to max_step in max-norm; freezes the pair when max|d| <= tol BEFORE the update (f and H are this round's).
// k_ev_nodes<K>: one thread per (cell, clone): the Cholesky factor of H in closed form, laplace = f* - sum log diag L, psi_q = psi* + L^-T z_q for every node.
// k_ev_reduce<K>: one thread per (cell, clone): f(psi_q) for q ascending, log sum_q w_q exp(f_q - f* + |z_q|^2 / 2) under a running maximum.
// No atomics; every sum has a fixed order: two calls agree bit for bit, and a pair's outputs depend on its cell's row alone.
// Batch-local slabs, the cell index fastest (a wave's loads and stores are 512 contiguous bytes): ps[slot * K + k][cell], zpart[chunk][slot * NMk + j][cell],
// mpart[chunk][slot][cell], and per pair fz / f* / H / rounds / conv as [clone (* entry)][cell].

#define CA_EV_QMAX 64     // quadrature nodes per call
#define CA_EV_LIVE 0      // a pair's state: still moving,
#define CA_EV_FROZEN 1    //   stopped (converged or not),
#define CA_EV_DEAD 2      //   A = -inf: never evaluated

template <int NS, int K, bool FULL>
__global__ void __launch_bounds__(CA_TB) __attribute__((amdgpu_waves_per_eu(NS * (FULL ? ca_proj_nm<K>::value : 1) <= 24 ? 4 : 3, NS * (FULL ? ca_proj_nm<K>::value : 1) <= 24 ? 4 : 3)))
k_ev_mom(const double* __restrict__ Ut /*[N][CA_LL_DMAX]: 0 | x, zero padded*/, const double* __restrict__ Vt /*[Gp][CA_LL_DMAX]: W | beta, zero padded*/,
         const double* __restrict__ Ec /*[Gp][C]*/, const double* __restrict__ ps /*[nslot * K][n_cnt]*/, const unsigned char* __restrict__ fz /*[C][n_cnt]*/,
         double* __restrict__ zpart /*[nzc][nslot * NMk][n_cnt]*/, double* __restrict__ mpart /*[nzc][nslot][n_cnt]*/, int64_t n_lo, int64_t n_cnt, int G, int C,
         int Q /* slots per clone */, int nslot) {
  constexpr int NMk = FULL ? ca_proj_nm<K>::value : 1;
  static_assert(K >= 1 && K <= CA_PROJ_KMAX, "");
  const int64_t li = (int64_t)blockIdx.x * CA_TB + threadIdx.x;
  const bool valid = li < n_cnt;
  const int64_t lc = valid ? li : n_cnt - 1;
  const int64_t n = n_lo + lc;
  const int s_lo = blockIdx.z * NS;   // wave-uniform; s_lo < nslot by the grid
  int cs[NS];                         // the slots' clones (wave-uniform; a slot past the end repeats the last clone and is never stored)
#pragma unroll
  for (int s = 0; s < NS; ++s) { const int sl = s_lo + s < nslot ? s_lo + s : nslot - 1; cs[s] = sl / Q; }
  bool live = false;
  if (valid) {
    const int c_lo = cs[0], c_hi = cs[NS - 1];
    for (int c = c_lo; c <= c_hi; ++c) { const unsigned char f = fz[(int64_t)c * n_cnt + lc]; live = live || (FULL ? f == CA_EV_LIVE : f != CA_EV_DEAD); }
  }
  if (!__any(live)) return;
  const int zc = blockIdx.y;
  const int g_lo = zc * CA_LL_ZCHUNK, g_hi = (g_lo + CA_LL_ZCHUNK < G) ? g_lo + CA_LL_ZCHUNK : G;   // wave-uniform
  double x[CA_LL_DMAX - K], p[NS * K];
#pragma unroll
  for (int d = K; d < CA_LL_DMAX; ++d) x[d - K] = Ut[n * CA_LL_DMAX + d];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int sl = s_lo + s < nslot ? s_lo + s : nslot - 1;
#pragma unroll
    for (int k = 0; k < K; ++k) p[s * K + k] = ps[((int64_t)sl * K + k) * n_cnt + lc];
  }
  auto xb_of = [&](const double* __restrict__ v) {   // the covariates' part of the exponent: once per (cell, gene)
    double e = 0.0;
#pragma unroll
    for (int d = K; d < CA_LL_DMAX; ++d) e = fma(x[d - K], v[d], e);
    return e;
  };
  auto eta_of = [&](int s, double xb, const double* __restrict__ v) {
    double e = xb;
#pragma unroll
    for (int k = 0; k < K; ++k) e = fma(p[s * K + k], v[k], e);
    return e;
  };
  double m[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) m[s] = -__builtin_inf();
  for (int g = g_lo; g < g_hi; ++g) {
    const double* __restrict__ v = Vt + (int64_t)g * CA_LL_DMAX;
    const double xb = xb_of(v);
#pragma unroll
    for (int s = 0; s < NS; ++s) m[s] = fmax(m[s], eta_of(s, xb, v));
  }
  double acc[NS * NMk];
#pragma unroll
  for (int i = 0; i < NS * NMk; ++i) acc[i] = 0.0;
  for (int g = g_lo; g < g_hi; ++g) {
    const double* __restrict__ v = Vt + (int64_t)g * CA_LL_DMAX;
    const double* __restrict__ er = Ec + (int64_t)g * C;
    const double xb = xb_of(v);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const double e = er[cs[s]];
      double w[NMk];   // e, e W_k, e W_k W_l (k <= l)
      w[0] = exp(eta_of(s, xb, v) - m[s]);
      if constexpr (FULL) {
        w[1] = w[0] * v[0];
        if constexpr (K == 1) { w[2] = w[1] * v[0]; }
        if constexpr (K == 2) { w[2] = w[0] * v[1]; w[3] = w[1] * v[0]; w[4] = w[1] * v[1]; w[5] = w[2] * v[1]; }
      }
#pragma unroll
      for (int j = 0; j < NMk; ++j) acc[s * NMk + j] = fma(e, w[j], acc[s * NMk + j]);
    }
  }
  if (live) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int sl = s_lo + s;
      if (sl < nslot) {
#pragma unroll
        for (int j = 0; j < NMk; ++j) zpart[((int64_t)zc * nslot * NMk + (int64_t)sl * NMk + j) * n_cnt + li] = acc[s * NMk + j];
        mpart[((int64_t)zc * nslot + sl) * n_cnt + li] = m[s];
      }
    }
  }
}

// the value of f at a slot's psi from its merged Z0: A + psi . B[:K] + x . B[K:] - s (m + log Z0) - |psi|^2 / 2 (ONE routine: the mode's value and a node's value
// at the same psi are the same bits)
template <int K>
__device__ __forceinline__ double ca_ev_f(double a, const double* psi, const double* __restrict__ Bn /*[CA_LL_DMAX]*/, double xB, double s, double m, double z0) {
  double ub = xB, q = 0.0;
#pragma unroll
  for (int k = 0; k < K; ++k) { ub = fma(psi[k], Bn[k], ub); q = fma(psi[k], psi[k], q); }
  double f = a + ub;
  if (s > 0.0) f -= s * (m + log(z0));   // (a cell without counts: every term is 0)
  return f - 0.5 * q;
}

// x . B[K:] of a cell (ascending; the padding is zero)
template <int K>
__device__ __forceinline__ double ca_ev_xb(const double* __restrict__ Un, const double* __restrict__ Bn) {
  double e = 0.0;
#pragma unroll
  for (int d = K; d < CA_LL_DMAX; ++d) e = fma(Un[d], Bn[d], e);
  return e;
}

template <int K>
__global__ void __launch_bounds__(CA_TB) k_ev_init(const double* __restrict__ A /*[N][C]*/, const double* __restrict__ Ut /*[N][CA_LL_DMAX]: start | x*/,
                                                   double* __restrict__ ps /*[C * K][n_cnt]*/, unsigned char* __restrict__ fz, int* __restrict__ rounds,
                                                   unsigned char* __restrict__ conv, double* __restrict__ fstar, double* __restrict__ Hm /*[C * NH][n_cnt]*/,
                                                   double* __restrict__ ev, double* __restrict__ lap, int64_t n_lo, int64_t n_cnt, int C) {
  constexpr int NH = K * (K + 1) / 2;
  const int64_t i = (int64_t)blockIdx.x * CA_TB + threadIdx.x;
  if (i >= n_cnt * C) return;
  const int c = (int)(i / n_cnt);
  const int64_t li = i - (int64_t)c * n_cnt, n = n_lo + li;
  const bool dead = !(A[n * C + c] > -__builtin_inf());
#pragma unroll
  for (int k = 0; k < K; ++k) ps[((int64_t)c * K + k) * n_cnt + li] = Ut[n * CA_LL_DMAX + k];
  fz[i] = dead ? CA_EV_DEAD : CA_EV_LIVE;
  rounds[i] = 0;
  conv[i] = 0;
  fstar[i] = -__builtin_inf();
  ev[i] = -__builtin_inf();
  lap[i] = -__builtin_inf();
  Hm[((int64_t)c * NH) * n_cnt + li] = 1.0;
  if constexpr (K == 2) { Hm[((int64_t)c * NH + 1) * n_cnt + li] = 0.0; Hm[((int64_t)c * NH + 2) * n_cnt + li] = 1.0; }
}

// One Newton round's finisher (final = 0), or the closing evaluation of the pairs that never froze (final = 1: no step, f and H at the psi they hold).
template <int K>
__global__ void __launch_bounds__(CA_TB) k_ev_step(const double* __restrict__ zpart, const double* __restrict__ mpart, const double* __restrict__ A,
                                                   const double* __restrict__ B /*[N][CA_LL_DMAX]*/, const double* __restrict__ Ut, const double* __restrict__ s64,
                                                   double* __restrict__ ps, unsigned char* __restrict__ fz, int* __restrict__ rounds, unsigned char* __restrict__ conv,
                                                   double* __restrict__ fstar, double* __restrict__ Hm, int64_t n_lo, int64_t n_cnt, int C, int nzc, int round,
                                                   int final, double tol, double max_step) {
  constexpr int NM = ca_proj_nm<K>::value;
  constexpr int NH = K * (K + 1) / 2;
  const int64_t i = (int64_t)blockIdx.x * CA_TB + threadIdx.x;
  if (i >= n_cnt * C) return;
  if (fz[i] != CA_EV_LIVE) return;
  const int c = (int)(i / n_cnt);
  const int64_t li = i - (int64_t)c * n_cnt, n = n_lo + li;
  double z[NM];
  const double m = ca_ll_merge<NM>(mpart + (int64_t)c * n_cnt + li, (int64_t)C * n_cnt, zpart + (int64_t)c * NM * n_cnt + li, (int64_t)C * NM * n_cnt, n_cnt, nullptr, 0, nzc, z);
  const double s = s64[n];
  const double* __restrict__ Bn = B + n * CA_LL_DMAX;
  double psi[K], h[NH], g[K], d[K], dmax;
#pragma unroll
  for (int k = 0; k < K; ++k) psi[k] = ps[((int64_t)c * K + k) * n_cnt + li];
  const double f = ca_ev_f<K>(A[n * C + c], psi, Bn, ca_ev_xb<K>(Ut + n * CA_LL_DMAX, Bn), s, m, z[0]);
  if constexpr (K == 1) {
    const double mu = z[1] / z[0];
    g[0] = Bn[0] - s * mu - psi[0];
    h[0] = 1.0 + s * (z[2] / z[0] - mu * mu);
    d[0] = g[0] / h[0];
    dmax = fabs(d[0]);
  } else {
    const double m0 = z[1] / z[0], m1 = z[2] / z[0];
    g[0] = Bn[0] - s * m0 - psi[0];
    g[1] = Bn[1] - s * m1 - psi[1];
    h[0] = 1.0 + s * (z[3] / z[0] - m0 * m0);
    h[1] = s * (z[4] / z[0] - m0 * m1);
    h[2] = 1.0 + s * (z[5] / z[0] - m1 * m1);
    const double det = h[0] * h[2] - h[1] * h[1];
    d[0] = (h[2] * g[0] - h[1] * g[1]) / det;
    d[1] = (h[0] * g[1] - h[1] * g[0]) / det;
    dmax = fmax(fabs(d[0]), fabs(d[1]));
  }
  bool stop = final != 0, ok = false;
  int used = round;
  if (!stop) {
    used = round + 1;
    if (!(dmax < __builtin_inf())) stop = true;   // a step that is no number: the pair stops where it is, not converged
    else if (dmax <= tol) { stop = true; ok = true; }
    else {
      const double sc = dmax > max_step ? max_step / dmax : 1.0;
#pragma unroll
      for (int k = 0; k < K; ++k) ps[((int64_t)c * K + k) * n_cnt + li] = psi[k] + d[k] * sc;
    }
  }
  if (!stop) return;
  fz[i] = CA_EV_FROZEN;
  rounds[i] = used;
  conv[i] = ok ? 1 : 0;
  fstar[i] = f;
#pragma unroll
  for (int j = 0; j < NH; ++j) Hm[((int64_t)c * NH + j) * n_cnt + li] = h[j];
}

// Laplace value and the nodes' psi of every possible pair: H = L L^T in closed form, psi_q = psi* + L^-T z_q
template <int K>
__global__ void __launch_bounds__(CA_TB) k_ev_nodes(const double* __restrict__ ps /*[C * K][n_cnt]*/, const unsigned char* __restrict__ fz, const double* __restrict__ fstar,
                                                    const double* __restrict__ Hm, const double* __restrict__ nodes /*[Q][K]*/, double* __restrict__ pq /*[C * Q * K][n_cnt]*/,
                                                    double* __restrict__ lap, int64_t n_cnt, int C, int Q) {
  constexpr int NH = K * (K + 1) / 2;
  const int64_t i = (int64_t)blockIdx.x * CA_TB + threadIdx.x;
  if (i >= n_cnt * C) return;
  const int c = (int)(i / n_cnt);
  const int64_t li = i - (int64_t)c * n_cnt;
  const bool dead = fz[i] == CA_EV_DEAD;
  double psi[K];
#pragma unroll
  for (int k = 0; k < K; ++k) psi[k] = ps[((int64_t)c * K + k) * n_cnt + li];
  double l00 = 1.0, l10 = 0.0, l11 = 1.0;
  if (!dead) {
    l00 = sqrt(Hm[((int64_t)c * NH) * n_cnt + li]);
    double hld = log(l00);
    if constexpr (K == 2) {
      l10 = Hm[((int64_t)c * NH + 1) * n_cnt + li] / l00;
      l11 = sqrt(Hm[((int64_t)c * NH + 2) * n_cnt + li] - l10 * l10);
      hld += log(l11);
    }
    lap[i] = fstar[i] - hld;
  }
  for (int q = 0; q < Q; ++q) {   // (a dead pair's nodes sit at its start: finite operands for the moment kernel, never reduced)
    const int64_t sl = (int64_t)c * Q + q;
    if constexpr (K == 1) pq[sl * n_cnt + li] = dead ? psi[0] : psi[0] + nodes[q] / l00;
    else {
      const double y1 = nodes[q * 2 + 1] / l11, y0 = (nodes[q * 2] - l10 * y1) / l00;
      pq[(sl * 2) * n_cnt + li] = dead ? psi[0] : psi[0] + y0;
      pq[(sl * 2 + 1) * n_cnt + li] = dead ? psi[1] : psi[1] + y1;
    }
  }
}

// evidence = laplace + log sum_q w_q exp(f(psi_q) - f* + |z_q|^2 / 2), q ascending under a running maximum
template <int K>
__global__ void __launch_bounds__(CA_TB) k_ev_reduce(const double* __restrict__ zpart /*[nzc][C * Q][n_cnt]*/, const double* __restrict__ mpart, const double* __restrict__ A,
                                                     const double* __restrict__ B, const double* __restrict__ Ut, const double* __restrict__ s64,
                                                     const double* __restrict__ pq, const unsigned char* __restrict__ fz, const double* __restrict__ fstar,
                                                     const double* __restrict__ lap, const double* __restrict__ nodes, const double* __restrict__ wts,
                                                     double* __restrict__ ev, int64_t n_lo, int64_t n_cnt, int C, int Q, int nzc) {
  const int64_t i = (int64_t)blockIdx.x * CA_TB + threadIdx.x;
  if (i >= n_cnt * C) return;
  if (fz[i] == CA_EV_DEAD) return;
  const int c = (int)(i / n_cnt);
  const int64_t li = i - (int64_t)c * n_cnt, n = n_lo + li;
  const int64_t nslot = (int64_t)C * Q;
  const double s = s64[n], a = A[n * C + c], f0 = fstar[i];
  const double* __restrict__ Bn = B + n * CA_LL_DMAX;
  const double xB = ca_ev_xb<K>(Ut + n * CA_LL_DMAX, Bn);
  double M = -__builtin_inf(), S = 0.0;
  for (int q = 0; q < Q; ++q) {
    const int64_t sl = (int64_t)c * Q + q;
    double z0[1];
    const double m = ca_ll_merge<1>(mpart + sl * n_cnt + li, nslot * n_cnt, zpart + sl * n_cnt + li, nslot * n_cnt, 0, nullptr, 0, nzc, z0);
    double psi[K], zz = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) { psi[k] = pq[(sl * K + k) * n_cnt + li]; zz = fma(nodes[q * K + k], nodes[q * K + k], zz); }
    const double t = ca_ev_f<K>(a, psi, Bn, xB, s, m, z0[0]) - f0 + 0.5 * zz;
    if (t > M) { S *= exp(M - t); M = t; }
    S = fma(wts[q], exp(t - M), S);
  }
  ev[i] = lap[i] + (M + log(S));
}
