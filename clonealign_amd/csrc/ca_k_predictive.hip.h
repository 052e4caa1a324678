// ca_k_predictive.hip.h -- part of ca_kernels.hip.h (textually included there, after ca_k_simulate.hip.h): replicate rows of ca_simulate_counts REDUCED WHERE
// THEY ARE DRAWN (ca_predictive_stats; include/clonealign_hip.h states the outputs).  For r = 0 .. n_rep - 1 the row y^(r)_n is the one k_simulate draws at
// draw = draw0 + r -- same table, same Philox counters, same search -- but it never leaves the block: what is stored is
//   ll[n][r]      = lgamma(total_n + 1) - sum_g lgamma(y_g + 1) + sum over y_g > 0 of y_g (log E[g][c_n] + eta_g - m - log Z_n)      one float64 per (cell, replicate)
//   T[r][c_n][g] += y_g                                                                                                              int64, integer atomics
// One launch, k_predictive: A BLOCK OWNS A CELL and walks the batch's cells with the grid's stride.  Per cell:
//   1. / 2. the shift m and the cumulative table: k_simulate's own steps 1 and 2 (the routine both kernels call, in ca_k_simulate.hip.h), ONCE for all n_rep
//      replicates -- the table costs G exp, as much as one replicate's draws at about 5000 counts per cell.  On the way
//      log w_g = log E + eta_g - m (not log(exp(...))) goes to the block's slab in global memory: a thread reads back exactly the genes it wrote.
//   per replicate:
//   3. the draws of k_simulate over ALL the cell's Philox blocks b = j >> 1 (k_simulate's work items cut the same sequence at multiples of CA_SIM_SEG), the
//      counters raised by integer atomics in the LDS histogram -- or, where it does not fit beside the table, in the block's row in global memory;
//   4. barrier; a thread walks its genes g = tid, tid + 1024, ...: reads AND CLEARS the counter (the histogram is zero again for the next replicate), adds
//      y log w - y log Z and lgamma(y + 1) (256-entry LDS table as in ca_k_loglik.hip.h, the routine itself above it), raises T for y > 0;
//   5. the block's sum in a fixed order: a thread's genes ascending, the wave by shuffles, the sixteen waves ascending by one lane, which stores ll[n][r].
// No float atomics, so two calls agree bit for bit; a cell's ll depends on its own inputs and (seed, draw0 + r, q) alone -- not on the grid, the batch or
// n_rep.  T is integer: exact under any order of arrival.
// LDS per block: k_simulate's plan (sim_plan) for the table and the histogram, plus 2.4 KB static (the lgamma table and the exchange arrays).
// Global scratch per block: G float64 of log w; with S > 1 G float64 of table; without an LDS histogram G int32 of counters (zeroed by the host once, kept
// zero by step 4).  The counters in global memory are touched by atomics alone (add in step 3, exchange with 0 in step 4): they are served by L2, never by
// a line of L1 that an atomic went past.

// Waves per SIMD the register budget is set for: 8 = two blocks of 1024 threads per CU, k_simulate's residency (the draws wait on dependent LDS reads, which a
// second block hides), at 64 registers and some scratch; 4 = one block per CU at up to 128 registers.  DESIGN section 7 has both forms' resource usage and times.
#ifndef CA_PRED_WAVES_PER_SIMD
#define CA_PRED_WAVES_PER_SIMD 8
#endif
__global__ void __launch_bounds__(CA_SIM_TB, CA_PRED_WAVES_PER_SIMD)
k_predictive(const double* __restrict__ Et /*[C][G]*/, const double* __restrict__ Vt /*[D][G]*/, const double* __restrict__ U /*[cells][D]*/,
             const int32_t* __restrict__ clone /*[cells]*/, const int64_t* __restrict__ total /*[cells]*/, const double* __restrict__ lgtab /*[CA_LL_LGTAB]*/,
             double* cum_blk /*[blocks][G] when S > 1*/, double* lw_blk /*[blocks][G]*/, int32_t* row_blk /*[blocks][G], zero, without an LDS histogram*/,
             double* __restrict__ ll /*[cells][n_rep]*/, unsigned long long* T /*[n_rep][C][G], or null*/, int64_t n_cnt, int G, int C, int D, int S, int nco,
             int hist_lds, uint32_t k0, uint32_t k1, uint64_t draw0, int n_rep, uint64_t q0 /* global index of the batch's first cell */) {
  extern __shared__ double sim_sm[];
  __shared__ double x_sum[CA_SIM_WAVES], x_max[CA_SIM_WAVES], x_red[CA_SIM_WAVES];
  __shared__ double lgt[CA_LL_LGTAB];
  double* co = sim_sm;                                        // [nco]: cum[min((k + 1) S, G) - 1]
  int* hist = reinterpret_cast<int*>(sim_sm + nco);           // [G] when hist_lds
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double* cg = cum_blk ? cum_blk + (size_t)blockIdx.x * G : nullptr;
  double* lw = lw_blk + (size_t)blockIdx.x * G;
  int32_t* row = hist_lds ? nullptr : row_blk + (size_t)blockIdx.x * G;
  for (int i = tid; i < CA_LL_LGTAB; i += CA_SIM_TB) lgt[i] = lgtab[i];
  if (hist_lds)
    for (int g = tid; g < G; g += CA_SIM_TB) hist[g] = 0;

  for (int64_t cell = blockIdx.x; cell < n_cnt; cell += gridDim.x) {
    const int64_t tot = total[cell];
    if (tot == 0) {   // (block-uniform) nothing is drawn: exactly 0, and nothing for T
      for (int r = tid; r < n_rep; r += CA_SIM_TB) ll[cell * n_rep + r] = 0.0;
      continue;
    }
    __syncthreads();   // the previous cell's table is no longer searched; the first cell: lgt and the zeroed histogram are complete
    const int cl = clone[cell];
    const double cum_all = sim_table<true>(Et + (size_t)cl * G, U + cell * D, Vt, co, cg, lw, x_sum, x_max, G, D, S);
    const double t_max = __longlong_as_double(__double_as_longlong(cum_all) - 1);   // the largest double below cum[G - 1] (> 0: the host refused an all-zero clone)
    const double log_z = log(cum_all);
    const double lg_tot = ca_ll_lgamma1p((double)tot);
    const uint64_t q = q0 + (uint64_t)cell;
    const int64_t nblk = (tot + 1) >> 1;
    for (int r = 0; r < n_rep; ++r) {
      const sim_ctr ctr = sim_counter(q, draw0 + (uint64_t)r);
      // 3. the draws (k_simulate's step 3 / 4 over every Philox block of the cell)
      for (int64_t i = tid; i < nblk; i += CA_SIM_TB) {
        uint32_t r4[4];
        sim_philox((uint32_t)i, ctr.c1, ctr.c2, ctr.c3, k0, k1, r4);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          if (2 * i + h >= tot) break;
          const int g = sim_gene(r4[2 * h], r4[2 * h + 1], cum_all, t_max, co, nco, cg, G, S);
          if (hist_lds) atomicAdd(&hist[g], 1);
          else atomicAdd(&row[g], 1);
        }
      }
      __syncthreads();
      // 4. the row's statistic, gene by gene; the counters are left at zero
      double acc = 0.0, lg = 0.0;
      unsigned long long* Trow = T ? T + ((size_t)r * C + cl) * G : nullptr;
      for (int g = tid; g < G; g += CA_SIM_TB) {
        int y;
        if (hist_lds) {
          y = hist[g];
          if (y) hist[g] = 0;
        } else {
          y = atomicExch(&row[g], 0);
        }
        if (y) {
          const double yd = (double)y;
          acc += yd * (lw[g] - log_z);
          lg += y < CA_LL_LGTAB ? lgt[y] : ca_ll_lgamma1p(yd);
          if (Trow) atomicAdd(&Trow[g], (unsigned long long)y);
        }
      }
      // 5. the block's sum, in a fixed order
      double v = acc - lg;
      for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
      if (lane == 0) x_red[wave] = v;
      __syncthreads();   // (also: every counter is zero again before the next replicate's draws)
      if (tid == 0) {
        double s = x_red[0];
        for (int k = 1; k < CA_SIM_WAVES; ++k) s += x_red[k];
        ll[cell * n_rep + r] = lg_tot + s;
      }
    }
  }
}
