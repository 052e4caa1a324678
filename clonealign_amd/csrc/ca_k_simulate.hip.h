// ca_k_simulate.hip.h -- part of ca_kernels.hip.h (textually included there, after ca_k_project.hip.h): count rows DRAWN from a fitted model,
//   y_n ~ Multinomial(total_n, p_n),  p_ng ~ E[g][clone_n] exp(U_n . V_g)      (ca_simulate_counts; include/clonealign_hip.h has the sampler, step by step).
// The model's generative direction; no count matrix is read.  One launch, k_simulate:
//
// A BLOCK OWNS ONE WORK ITEM = one cell's draws [j_lo, j_lo + CA_SIM_SEG) (the host lists the items; a cell of up to CA_SIM_SEG draws is one item, a cell of
// 200 000 is thirteen, so a launch is never serialised behind its largest cell).  Per item:
//   1. m = max of eta_g = U_n . V_g over the genes with E > 0 (one pass, wave shuffles + one LDS exchange);
//   2. w_g = E exp(eta_g - m) and its inclusive scan, CA_SIM_TB genes per tile: a wave scan, the wave totals through LDS, a running carry.  The grouping of
//      the float64 sums is therefore the scan's, not a sequential one.  A scan in floating point need not be monotone in g, so the table kept is the running
//      MAXIMUM of the scanned values over the genes with w > 0 (a second scan; max is exact under any grouping): non-decreasing, and a gene with w = 0 has
//      exactly its predecessor's value and is never drawn.  Every S-th value (and the last) goes to LDS; with S > 1 the full table goes to global memory (the
//      cell's slab: every item of a cell writes the same bits);
//   3. draws: a lane takes Philox block b = j >> 1 (two draws), forms u on 53 bits, t = u * cum[G - 1], and finds the first g with cum[g] > t by a
//      branch-free binary search over the LDS table (ceil(log2(G / S)) dependent LDS reads), then over its S-gene group in global memory (L1 / L2);
//   4. the gene's counter is raised by an INTEGER atomic -- in an LDS histogram of the row where it fits beside the table, else on the int32 row itself.
//      Integer addition commutes and every draw has its own counter, so the atomics cannot change a bit of the result: unlike the float64 sums everywhere
//      else in this library (fixed order, no atomics), the order of arrival is not observable here.  The histogram is then stored (the cell's only item) or
//      added to the zeroed row (one of several items).
// LDS per block: 8 * ceil(G / S) + 4 * G (histogram, when it fits) <= CA_SIM_LDS bytes; S and the histogram's place are the host's pick (sim_plan).
// Steps 1 and 2 (sim_table) and one draw of step 3 (sim_counter, sim_gene) are routines of this file that k_predictive (ca_k_predictive.hip.h) calls too.

#define CA_SIM_TB 1024        // threads per block: two blocks fill a CU's 32 waves at the LDS budget below
#define CA_SIM_SEG 16384      // draws per work item (even: an item starts on a Philox block)
#define CA_SIM_LDS 61440      // dynamic LDS per block for the table and the histogram (two blocks per CU beside the static exchange arrays)
#define CA_SIM_WAVES (CA_SIM_TB / 64)

struct ca_sim_item { int32_t cell; uint32_t j_lo; };   // cell: index inside the launch's batch; j_lo: first draw, a multiple of CA_SIM_SEG

// Philox4x32-10 (Salmon et al., SC'11): the function of philox_host.h / rng.py
__device__ __forceinline__ void sim_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// eta = sum_d U[d] V[d][g], products and sums rounded one by one in ascending d (no fused multiply-add: the host restatement's bits)
__device__ __forceinline__ double sim_eta(const double* __restrict__ u, const double* __restrict__ Vt, int D, int G, int g) {
  double e = 0.0;
#pragma unroll 1
  for (int d = 0; d < D; ++d) {   // (u[d] is a scalar load per step: no register array)
    const double p = __dmul_rn(u[d], Vt[(size_t)d * G + g]);
    e = d == 0 ? p : __dadd_rn(e, p);
  }
  return e;
}

// first index in [0, len) whose table value exceeds t; the caller guarantees one exists (branch-free: every lane runs the same steps, indices stay inside)
__device__ __forceinline__ int sim_search(const double* tab, int len, double t) {
  int lo = 0;
  while (len > 1) {
    const int half = len >> 1;
    lo += (tab[lo + half - 1] <= t) ? half : 0;
    len -= half;
  }
  return lo;
}

// The Philox counter words of cell q's draws at stream `draw`; word 0 is the block index b = j >> 1, filled in by the caller's loop.
struct sim_ctr { uint32_t c1, c2, c3; };
__device__ __forceinline__ sim_ctr sim_counter(uint64_t q, uint64_t draw) {
  return sim_ctr{(uint32_t)q, (uint32_t)draw, (uint32_t)((draw >> 32) & 0xFFFFu) | ((uint32_t)(q >> 32) << 16)};
}

// Step 3 for one draw: the gene of the 64-bit half (lo, hi) of a Philox block -- u on 53 bits, t = min(u cum[G - 1], t_max), the search in co (LDS) and,
// with S > 1, in the gene's S-gene group of cg.
__device__ __forceinline__ int sim_gene(uint32_t lo, uint32_t hi, double cum_all, double t_max, const double* co, int nco, const double* cg, int G, int S) {
  const uint64_t x = ((uint64_t)hi << 21) | (uint64_t)(lo >> 11);
  const double uu = ((double)x + 0.5) * 0x1p-53;
  const double t = fmin(uu * cum_all, t_max);
  int g = sim_search(co, nco, t);
  if (S > 1) {
    const int gb = g * S;
    g = gb + sim_search(cg + gb, (G - gb < S) ? G - gb : S, t);
  }
  return g;
}

// Steps 1 and 2 for one cell, called by every thread of a CA_SIM_TB block: the table in co (LDS) and cg (S > 1); returns cum[G - 1].  k_simulate and k_predictive
// both draw from THIS table, which is what makes the latter's replicate rows the former's rows bit for bit.  LW: log w_g = log E + eta_g - m also goes to lw
// (k_predictive's statistic; w itself has the same bits either way).
template <bool LW>
__device__ __forceinline__ double sim_table(const double* __restrict__ e, const double* __restrict__ u, const double* __restrict__ Vt, double* co, double* cg,
                                            double* lw, double* x_sum, double* x_max, int G, int D, int S) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // 1. the shift: the largest exponent over the genes that can be drawn
  double m = -HUGE_VAL;
  if (D > 0) {
    for (int g = tid; g < G; g += CA_SIM_TB)
      if (e[g] > 0.0) m = fmax(m, sim_eta(u, Vt, D, G, g));
    for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off));
    if (lane == 0) x_max[wave] = m;
    __syncthreads();
    m = x_max[0];
    for (int k = 1; k < CA_SIM_WAVES; ++k) m = fmax(m, x_max[k]);
    __syncthreads();
  } else {
    m = 0.0;
  }
  // 2. weights, their inclusive scan and the running maximum that makes it a table
  double carry = 0.0, top = 0.0;   // block-uniform: the sum and the table value before this tile
  for (int base = 0; base < G; base += CA_SIM_TB) {
    const int g = base + tid;
    double w = 0.0;
    if (g < G) {
      const double eg = e[g];
      if (LW) {
        double l = 0.0;
        if (eg > 0.0) {
          if (D > 0) {
            const double x = sim_eta(u, Vt, D, G, g) - m;
            w = eg * exp(x);
            l = log(eg) + x;
          } else {
            w = eg;
            l = log(eg);
          }
        }
        lw[g] = l;
      } else if (eg > 0.0) {
        w = D > 0 ? eg * exp(sim_eta(u, Vt, D, G, g) - m) : eg;
      }
    }
    double s = w;
    for (int off = 1; off < 64; off <<= 1) {
      const double v = __shfl_up(s, off);
      if (lane >= off) s += v;
    }
    if (lane == 63) x_sum[wave] = s;
    __syncthreads();
    double before = 0.0, all = 0.0;
#pragma unroll 1
    for (int k = 0; k < CA_SIM_WAVES; ++k) {
      if (k == wave) before = all;
      all += x_sum[k];
    }
    const double r = carry + (before + s);
    carry += all;
    double c = w > 0.0 ? r : 0.0;   // (every table value is >= 0, so 0 is the maximum's identity)
    for (int off = 1; off < 64; off <<= 1) {
      const double v = __shfl_up(c, off);
      if (lane >= off) c = fmax(c, v);
    }
    if (lane == 63) x_max[wave] = c;
    __syncthreads();
    double tile = top;
#pragma unroll 1
    for (int k = 0; k < CA_SIM_WAVES; ++k) {
      if (k == wave) c = fmax(c, tile);
      tile = fmax(tile, x_max[k]);
    }
    top = tile;
    if (g < G) {
      if (S == 1) {
        co[g] = c;
      } else {
        cg[g] = c;
        if (g % S == S - 1 || g == G - 1) co[g / S] = c;
      }
    }
  }
  __syncthreads();   // the table (LDS, and this block's own stores to its cell's slab) is complete
  return top;
}

__global__ void __launch_bounds__(CA_SIM_TB)
k_simulate(const double* __restrict__ Et /*[C][G]*/, const double* __restrict__ Vt /*[D][G]*/, const double* __restrict__ U /*[cells][D]*/,
           const int32_t* __restrict__ clone /*[cells]*/, const int64_t* __restrict__ total /*[cells]*/, const ca_sim_item* __restrict__ items,
           double* cumg /*[cells][G] when S > 1*/, int32_t* Y /*[cells][G], zeroed*/, int G, int D, int S, int nco, int hist_lds,
           uint32_t k0, uint32_t k1, uint64_t draw, uint64_t q0 /* global index of the batch's first cell */) {
  extern __shared__ double sim_sm[];
  __shared__ double x_sum[CA_SIM_WAVES], x_max[CA_SIM_WAVES];
  double* co = sim_sm;                                        // [nco]: cum[min((k + 1) S, G) - 1]
  int* hist = reinterpret_cast<int*>(sim_sm + nco);           // [G] when hist_lds
  const ca_sim_item it = items[blockIdx.x];
  const int tid = threadIdx.x;
  const int64_t cell = it.cell;
  double* cg = cumg ? cumg + (size_t)cell * G : nullptr;
  int32_t* yrow = Y + (size_t)cell * G;

  if (hist_lds)
    for (int g = tid; g < G; g += CA_SIM_TB) hist[g] = 0;
  // 1. / 2. the shift and the table (its closing barrier also completes the zeroed histogram)
  const double cum_all = sim_table<false>(Et + (size_t)clone[cell] * G, U + cell * D, Vt, co, cg, nullptr, x_sum, x_max, G, D, S);

  // 3. / 4. the draws
  const int64_t tot = total[cell];
  const int64_t left = tot - (int64_t)it.j_lo;
  const int cnt = (int)(left < CA_SIM_SEG ? left : CA_SIM_SEG);
  const bool only = tot <= CA_SIM_SEG;
  const double t_max = __longlong_as_double(__double_as_longlong(cum_all) - 1);   // the largest double below cum[G - 1] (> 0: the host refused an all-zero clone)
  const sim_ctr ctr = sim_counter(q0 + (uint64_t)cell, draw);
  const int nblk = (cnt + 1) >> 1;
  for (int i = tid; i < nblk; i += CA_SIM_TB) {
    uint32_t r4[4];
    sim_philox((it.j_lo >> 1) + (uint32_t)i, ctr.c1, ctr.c2, ctr.c3, k0, k1, r4);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (2 * i + h >= cnt) break;
      const int g = sim_gene(r4[2 * h], r4[2 * h + 1], cum_all, t_max, co, nco, cg, G, S);
      if (hist_lds) atomicAdd(&hist[g], 1);
      else atomicAdd(&yrow[g], 1);
    }
  }
  if (hist_lds) {
    __syncthreads();
    for (int g = tid; g < G; g += CA_SIM_TB) {
      const int v = hist[g];
      if (only) yrow[g] = v;
      else if (v) atomicAdd(&yrow[g], v);
    }
  }
}
