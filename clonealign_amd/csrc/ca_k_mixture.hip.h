// ca_k_mixture.hip.h -- part of ca_kernels.hip.h (textually included there, after ca_k_pairll.hip.h): the maximum-likelihood MIXTURE of all clones per cell
// (ca_clone_mixture; a spot, a bulk sample, a contaminated droplet, an off-grid doublet: the sum of multinomial rows of several clones is multinomial in
// sum_c pi_c p_n.c).  In the notation of ca_k_pairll.hip.h, per cell, with lz = min_c log Z_nc and q_gc = E_gc exp(lz - log Z_nc) (every factor <= 1):
//   mix_ll(pi) = sum_{g: y>0} y_g log m_g - s lz + base_n,   m_g = sum_c pi_c q_gc
//   g_c  = sum_{g: y>0} y_g q_gc / m_g            (sum_c pi_c g_c = s_eff, the counts on usable entries)
//   H_cd = sum_{g: y>0} y_g q_gc q_gd / m_g^2     (minus the Hessian)
//   bound = max_c g_c - sum_c pi_c g_c            (concavity: no pi' on the simplex beats mix_ll(pi) by more)
// maximised over the simplex by projected Newton on phi(pi) = f(pi) - s_eff sum_c pi_c over pi >= 0 (include/clonealign_hip.h has the round and the rules).
// Float64 throughout, no atomics.
//
// k_mix_list<YT>: A WAVE OWNS A CELL and compacts the row's non-zero counts in ascending gene order exactly as k_pair_ll does (one ballot per column of the
// lane's VEC, mbcnt over the lanes below, u8 escapes resolved here) -- but the list must outlive the segment, so (gene, y) go to a slab of the batch in global
// memory, up to Gp entries a cell, and the count to ln.
//
// k_mix_rounds: A WAVE OWNS A CELL AND LOOPS UNTIL ITS CELL STOPS; all rounds are in this one launch, and the kernel has no block barrier, so the waves of a
// block finish independently.  Per evaluation at pi:
//   the first pass, LANES OVER ENTRIES: a lane forms m of its entry from the gene's row of E compact (w_c = pi_c a_c in LDS), stores r = y / m and r^2 / y
//     beside the entry and adds y log m; the wave's sum is a fixed-order butterfly.  An entry with every q_gc = 0 is left out (mix_ll is -inf exactly);
//   the second pass, LANES ARE SLOTS: the C gradient slots and the C (C + 1) / 2 slots of the packed lower triangle of H.  The wave reads 64 entries with one
//     coalesced load each of (gene, r, r^2 / y), then walks them: the entry is wave-uniform (readlane), a lane loads E[g][c] and E[g][d] of its slot and adds
//     its slot alone, in ascending gene order.  More than 64 slots are further sweeps of the same wave over the list.
// Per round: gamma = g - s_eff, Bertsekas' active set, the C x C Cholesky solve in the wave's LDS on the packed triangle (active rows replaced by identity
// rows, so no index map; a lane owns a row, a column step per k: C^2 / 2 dependent updates, not C^3 / 6), the four trial points max(pi + t d, 0), t = 1, 1/2,
// 1/4, 1/8, evaluated in ONE pass over the list (lanes over entries, four logarithms an entry), Armijo, else one EM step; renormalise.
// A round keeps no state but pi: T rounds in one call are T calls of one round, bit for bit.
//
// Sums: every sum is in a fixed order that depends on the cell's row and the inputs only -- a lane's entries i = lane, lane + 64, ..., then the butterfly; a
// slot over the entries in ascending order; sums over clones sequentially from LDS.  Two calls agree bit for bit, and a cell's outputs depend neither on the
// cell range, nor on the batching, nor on its place in the launch.
#define CA_MIX_CMAX 32                                        // clones (extra profiles included)
#define CA_MIX_HP (CA_MIX_CMAX * (CA_MIX_CMAX + 1) / 2)       // packed lower triangle
#define CA_MIX_NV 13                                         // vectors of CA_MIX_CMAX doubles per wave

__device__ __forceinline__ void ca_mix_sync() {   // the wave's LDS accesses stay in order; this keeps the compiler from moving them across
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
}
__device__ __forceinline__ double ca_mix_sum(double v) {
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);   // (a + b = b + a bit for bit: every lane holds the same sum)
  return v;
}
__device__ __forceinline__ double ca_mix_max(double v) {
  for (int o = 1; o < 64; o <<= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double ca_mix_lane(double v, int l /* wave-uniform */) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

template <typename YT>
__global__ void __launch_bounds__(CA_TB) k_mix_list(const YT* __restrict__ Y, const int64_t* __restrict__ orowptr /* or null */, const int* __restrict__ ocol,
                                                    const float* __restrict__ oval, int* __restrict__ lg /*[n_cnt][Gp]*/, double* __restrict__ ly /*[n_cnt][Gp]*/,
                                                    int* __restrict__ ln /*[n_cnt]*/, int64_t n_lo, int64_t n_cnt, int G, int Gp, int nseg) {
  constexpr int VEC = YVec<YT>::VEC;
  constexpr int SEGW = 64 * VEC;   // columns per segment
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t li = (int64_t)blockIdx.x * (CA_TB / 64) + wave;   // the wave's cell of this batch
  if (li >= n_cnt) return;   // wave-uniform (the kernel has no block barrier)
  const int64_t n = n_lo + li;
  long long oe0 = 0; int noe = 0;
  if constexpr (sizeof(YT) == 1) {
    if (orowptr) { oe0 = orowptr[n]; noe = (int)(orowptr[n + 1] - oe0); }   // wave-uniform
  }
  typedef unsigned v4u_ __attribute__((ext_vector_type(4)));
  const char* row = reinterpret_cast<const char*>(Y) + n * ((int64_t)Gp * (int64_t)sizeof(YT)) + lane * 16;
  int* mg = lg + li * Gp;
  double* my = ly + li * Gp;
  int at = 0;   // entries so far (wave-uniform): at most the row's G <= Gp columns
  v4u_ nxt = __builtin_nontemporal_load(reinterpret_cast<const v4u_*>(row));
  for (int sg = 0; sg < nseg; ++sg) {
    const v4u_ cur = nxt;
    if (sg + 1 < nseg) nxt = __builtin_nontemporal_load(reinterpret_cast<const v4u_*>(row + (int64_t)(sg + 1) * SEGW * (int64_t)sizeof(YT)));
    float y[VEC];
    YVec<YT>::decode((uint4){cur.x, cur.y, cur.z, cur.w}, y);
    const int g0 = sg * SEGW + lane * VEC;
    // compaction in ascending gene order: this lane's entries start behind those of the lanes below
    int below = 0, total = 0;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const unsigned long long m = __builtin_amdgcn_ballot_w64(g0 + k < G && y[k] > 0.f);
      below += (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
      total += __builtin_popcountll(m);
    }
    total = __builtin_amdgcn_readfirstlane(total);
    int pos = at + below;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      if (g0 + k < G && y[k] > 0.f) {
        double yd = (double)y[k];
        if constexpr (sizeof(YT) == 1) {
          if (y[k] == 255.f && noe > 0) yd += ca_mse_excess(ocol, oval, oe0, noe, g0 + k);   // rare: 255 + an entry of the overflow list
        }
        my[pos] = yd;
        mg[pos] = g0 + k;
        ++pos;
      }
    }
    at += total;
  }
  if (lane == 0) ln[li] = at;
}

// packed lower triangle: (i, j), i >= j
__device__ __forceinline__ int ca_mix_tri(int i, int j) { return i * (i + 1) / 2 + j; }

__global__ void __launch_bounds__(CA_TB) k_mix_rounds(const double* __restrict__ Ec /*[G][C]*/, const double* __restrict__ lzc /*[n_cnt][C]*/, const double* __restrict__ base /*[n_cnt]*/,
                                                      const double* __restrict__ s64, const int* __restrict__ lg, const double* __restrict__ ly, double* lr, double* lq,
                                                      const int* __restrict__ ln, const double* __restrict__ start /*[n_cnt][C] or null: uniform*/,
                                                      double* __restrict__ w_out /*[n_cnt][C]*/, double* __restrict__ g_out /*[n_cnt][C]*/, double* __restrict__ mll,
                                                      double* __restrict__ bnd, int* __restrict__ rnd, int64_t n_lo, int64_t n_cnt, int Gp, int C, int max_iter, double tol) {
  __shared__ double sH[CA_TB / 64][CA_MIX_HP];
  __shared__ double sV[CA_TB / 64][CA_MIX_NV][CA_MIX_CMAX];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t li = (int64_t)blockIdx.x * (CA_TB / 64) + wave;   // the wave's cell of this batch
  if (li >= n_cnt) return;   // wave-uniform (the kernel has no block barrier)
  double* Hp = sH[wave];
  double* a = sV[wave][0];    // exp(lz - log Z_c)
  double* pi = sV[wave][1];
  double* w = sV[wave][2];    // pi_c a_c
  double* gv = sV[wave][3];   // g
  double* d = sV[wave][4];    // right-hand side, then the direction
  double* tr = sV[wave][5];   // [4][C]: the trial points
  double* tw = sV[wave][9];   // [4][C]: trial_c a_c
  const int cnt = __builtin_amdgcn_readfirstlane(ln[li]);
  const int* eg = lg + li * Gp;
  const double* ey = ly + li * Gp;
  double* er = lr + li * Gp;
  double* eq = lq + li * Gp;
  const bool mine = lane < C;   // this lane's clone
  const double lzl = mine ? lzc[li * C + lane] : HUGE_VAL;
  const double lz = -ca_mix_max(-lzl);
  const double al = mine ? exp(lz - lzl) : 0.0;
  if (mine) { a[lane] = al; pi[lane] = start ? start[li * C + lane] : 1.0 / (double)C; }
  ca_mix_sync();
  const int NS = C + C * (C + 1) / 2;
  int rounds = 0;
  bool restarted = false, ninf = false, bad = false;
  double f = 0.0, seff = 0.0, bound = 0.0;
  for (;;) {
    if (mine) w[lane] = pi[lane] * al;
    ca_mix_sync();
    // ---- the first pass, lanes over entries: m, r = y / m and r^2 / y beside the entry, y log m
    double accf = 0.0, accs = 0.0;
    int flg = 0;
    for (int i = lane; i < cnt; i += 64) {
      const double y = ey[i];
      const double* __restrict__ e = Ec + (int64_t)eg[i] * C;
      double m = 0.0, u = 0.0;
      for (int c = 0; c < C; ++c) { const double x = e[c]; m = fma(w[c], x, m); u = fma(a[c], x, u); }
      double r = 0.0, q = 0.0;
      if (u > 0.0) {
        accs += y;
        if (m > 0.0) { accf = fma(y, log(m), accf); r = y / m; q = r * r / y; }
        else flg |= 2;   // this pi's zeros exclude the entry
      } else flg |= 1;   // no clone supports the entry
      er[i] = r; eq[i] = q;
    }
    f = ca_mix_sum(accf);
    seff = ca_mix_sum(accs);
    ninf = __builtin_amdgcn_ballot_w64((flg & 1) != 0) != 0ull;
    bad = __builtin_amdgcn_ballot_w64((flg & 2) != 0) != 0ull;
    if (bad && max_iter > 0 && !restarted) {   // (a first evaluation only: no step leaves a usable entry without support)
      restarted = true;
      if (mine) pi[lane] = 1.0 / (double)C;
      ca_mix_sync();
      continue;
    }
    // ---- the second pass, lanes are slots (entry i is loaded by lane i % 64, the lane that stored it: no cross-lane traffic through memory)
    for (int s0 = 0; s0 < NS; s0 += 64) {
      const int slot = s0 + lane;
      const bool live = slot < NS;
      const int sl = live ? slot : 0;
      const bool isg = sl < C;
      int c = sl, dd = sl;
      if (!isg) {
        const int p = sl - C;
        c = 0;
        while ((c + 1) * (c + 2) / 2 <= p) ++c;
        dd = p - c * (c + 1) / 2;
      }
      const double ac = a[c], ad = a[dd];
      const double* __restrict__ ecp = Ec + c;
      const double* __restrict__ edp = Ec + dd;
      double acc = 0.0;
      for (int i0 = 0; i0 < cnt; i0 += 64) {
        const int idx = i0 + lane;
        const bool in = idx < cnt;
        const int gl = in ? eg[idx] : 0;
        const double rl = in ? er[idx] : 0.0, ql = in ? eq[idx] : 0.0;
        const int nn = cnt - i0 < 64 ? cnt - i0 : 64;
#pragma unroll 4
        for (int k = 0; k < nn; ++k) {
          const int64_t g = (int64_t)__builtin_amdgcn_readlane(gl, k) * C;   // wave-uniform
          const double r = ca_mix_lane(rl, k), q = ca_mix_lane(ql, k);
          const double xc = ecp[g] * ac, xd = edp[g] * ad;
          acc = isg ? fma(r, xc, acc) : fma(q * xc, xd, acc);
        }
      }
      if (live) {
        if (isg) gv[c] = acc;
        else Hp[sl - C] = acc;
      }
    }
    ca_mix_sync();
    double sg = 0.0, gmax = -HUGE_VAL, spi = 0.0;
    for (int c = 0; c < C; ++c) { sg = fma(pi[c], gv[c], sg); gmax = fmax(gmax, gv[c]); spi += pi[c]; }
    bound = seff > 0.0 ? (bad ? HUGE_VAL : fmax(gmax - sg, 0.0)) : 0.0;
    if (!(seff > 0.0) || bound <= tol || rounds >= max_iter) break;
    // ---- the round: gamma, the active set, the solve
    const double pc = mine ? pi[lane] : 0.0;
    const double gam = mine ? gv[lane] - seff : 0.0;
    const double hcc = mine ? Hp[ca_mix_tri(lane, lane)] : 0.0;
    const double term = mine ? (hcc > 0.0 ? fabs(pc - fmax(pc + gam / hcc, 0.0)) : pc) : 0.0;
    const double eps = fmin(1e-3, ca_mix_max(term));
    const bool active = mine && pc <= eps && gam < 0.0;
    const unsigned amask = (unsigned)__builtin_amdgcn_ballot_w64(active);   // wave-uniform (C <= 32)
    const int nF = C - __builtin_popcount(amask);
    double trF = 0.0;
    for (int c = 0; c < C; ++c)
      if (!((amask >> c) & 1u)) trF += Hp[ca_mix_tri(c, c)];
    const double ridge = nF > 0 ? 1e-12 * trF / (double)nF : 0.0;
    ca_mix_sync();
    if (mine) {
      d[lane] = active ? 0.0 : gam;
      for (int j = 0; j <= lane; ++j) {
        const int ix = ca_mix_tri(lane, j);
        if (active || ((amask >> j) & 1u)) Hp[ix] = j == lane ? 1.0 : 0.0;   // an identity row: the solve is that of the free set
        else if (j == lane) Hp[ix] += ridge;
      }
    }
    ca_mix_sync();
    bool fail = false;
    for (int k = 0; k < C; ++k) {   // right-looking Cholesky, a lane owns a row
      const double p = Hp[ca_mix_tri(k, k)];
      if (!(p > 0.0) || !(p < HUGE_VAL)) { fail = true; break; }   // wave-uniform
      const double l = sqrt(p);
      ca_mix_sync();
      if (lane == k) Hp[ca_mix_tri(k, k)] = l;
      else if (mine && lane > k) Hp[ca_mix_tri(lane, k)] /= l;
      ca_mix_sync();
      if (mine && lane > k) {
        const double lik = Hp[ca_mix_tri(lane, k)];
        for (int j = k + 1; j <= lane; ++j) Hp[ca_mix_tri(lane, j)] = fma(-lik, Hp[ca_mix_tri(j, k)], Hp[ca_mix_tri(lane, j)]);
      }
      ca_mix_sync();
    }
    if (!fail) {
      for (int k = 0; k < C; ++k) {   // L z = b
        const double z = d[k] / Hp[ca_mix_tri(k, k)];
        ca_mix_sync();
        if (lane == k) d[k] = z;
        else if (mine && lane > k) d[lane] = fma(-Hp[ca_mix_tri(lane, k)], z, d[lane]);
        ca_mix_sync();
      }
      for (int k = C - 1; k >= 0; --k) {   // L^T x = z
        const double x = d[k] / Hp[ca_mix_tri(k, k)];
        ca_mix_sync();
        if (lane == k) d[k] = x;
        else if (lane < k) d[lane] = fma(-Hp[ca_mix_tri(k, lane)], x, d[lane]);
        ca_mix_sync();
      }
    }
    const double dl = mine ? (active ? (hcc > 0.0 ? gam / hcc : -1.0) : d[lane]) : 0.0;
    if (__builtin_amdgcn_ballot_w64(!(fabs(dl) < HUGE_VAL)) != 0ull) fail = true;
    int pick = -1;
    if (!fail) {
      // ---- the line search: four trial points in one pass over the list
      if (mine) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const double v = fmax(fma(1.0 / (double)(1 << t), dl, pc), 0.0);
          tr[t * CA_MIX_CMAX + lane] = v;
          tw[t * CA_MIX_CMAX + lane] = v * al;
        }
      }
      ca_mix_sync();
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
      for (int i = lane; i < cnt; i += 64) {
        if (!(er[i] > 0.0)) continue;   // an entry left out
        const double y = ey[i];
        const double* __restrict__ e = Ec + (int64_t)eg[i] * C;
        double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0;
        for (int c = 0; c < C; ++c) {
          const double x = e[c];
          m0 = fma(tw[c], x, m0); m1 = fma(tw[CA_MIX_CMAX + c], x, m1); m2 = fma(tw[2 * CA_MIX_CMAX + c], x, m2); m3 = fma(tw[3 * CA_MIX_CMAX + c], x, m3);
        }
        a0 = fma(y, log(m0), a0); a1 = fma(y, log(m1), a1); a2 = fma(y, log(m2), a2); a3 = fma(y, log(m3), a3);   // (log 0 = -inf: the point is refused)
      }
      const double ft[4] = {ca_mix_sum(a0), ca_mix_sum(a1), ca_mix_sum(a2), ca_mix_sum(a3)};
      const double phi0 = f - seff * spi;
#pragma unroll
      for (int t = 3; t >= 0; --t) {
        double st = 0.0, gd = 0.0;
        for (int c = 0; c < C; ++c) { const double v = tr[t * CA_MIX_CMAX + c]; st += v; gd = fma(gv[c] - seff, v - pi[c], gd); }
        const double ph = ft[t] - seff * st;
        if (fabs(ph) < HUGE_VAL && ph >= phi0 + 1e-4 * gd) pick = t;   // (descending t: the largest step that passes stays)
      }
    }
    ca_mix_sync();
    double pn = 0.0;
    if (mine) {
      pn = pc * gv[lane] / seff;   // the EM step: never lowers f
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (pick == t) pn = tr[t * CA_MIX_CMAX + lane];
      pi[lane] = pn;
    }
    ca_mix_sync();
    double sum = 0.0;
    for (int c = 0; c < C; ++c) sum += pi[c];
    ca_mix_sync();
    if (mine && sum > 0.0 && sum < HUGE_VAL) pi[lane] = pn / sum;
    ca_mix_sync();
    ++rounds;
  }
  if (mine) {
    w_out[li * C + lane] = pi[lane];
    g_out[li * C + lane] = seff > 0.0 ? gv[lane] / seff : 0.0;
  }
  if (lane == 0) {
    const double s = s64[n_lo + li];
    double r = f + base[li];
    if (s > 0.0) r -= s * lz;   // (a cell without counts: every term is 0)
    mll[li] = (ninf || bad) ? -HUGE_VAL : r;
    bnd[li] = bound;
    rnd[li] = rounds;
  }
}
