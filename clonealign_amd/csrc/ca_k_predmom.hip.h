// ca_k_predmom.hip.h -- part of ca_kernels.hip.h (textually included there, after ca_k_predictive.hip.h): the moments of ca_predictive_stats's replicates IN
// CLOSED FORM (ca_predictive_moments; include/clonealign_hip.h states the outputs).  Given the clones and the row sums, a replicate row is one multinomial
// draw, so nothing has to be drawn: with p_ng = w_g / Z_n, w_g = E[g][c_n] exp(eta_g - m) and lp_g = log E + (eta_g - m) - log Z_n,
//   cell_mean[n] = total_n h,  h = sum_g p lp        cell_var[n] = total_n sum_g p (lp - h)^2                                   (the linear part of the log-likelihood)
//   T_mean / T_var / T_cum3 [g][c] = sum over the cells of clone c of total_n p,  total_n p (1 - p),  total_n p (1 - p)(1 - 2p)   (the pseudo-bulk totals)
// No count matrix is read.  Two phases (D > 0; without factors p depends on the clone alone and the host does the whole call):
//   k_predmom_loge   log E once per (clone, gene), so that every later log E is a load.
//   k_predmom_cell   A BLOCK OWNS A CELL and walks the batch's cells with the grid's stride.  Four passes over the cell's genes, a thread on g = tid, tid + 256,
//                    ...: (1) m = max of eta over E > 0 (k_simulate's step 1: sim_eta, the same roundings); (2) w_g, kept in the block's row -- LDS up to 7680
//                    genes, else the block's slab in global memory; a thread reads back exactly the genes it wrote --, the largest w and Z = (the sum of the
//                    others) + the largest; (3) h; (4) the centred variance.  A gene with p > 1/2 takes lp = log1p(-(the others' sum) / Z): where one gene
//                    holds nearly all of a cell, log E + x - log Z cancels to rounding noise of size 1e-16 while the true value may be 1e-20.
//                    One exp per (cell, gene).  Every sum in a fixed order: a thread's genes ascending, the wave by shuffles, the four waves ascending, so a
//                    cell's values depend on its own inputs alone.  Stores m_n and Z_n for the gene phase.
//   k_predmom_gene   the host lists the batch's cells with total > 0 sorted by clone (stable) and cuts the list into strips that never straddle a clone.  A
//                    BLOCK OWNS 256 GENES x ONE STRIP, A LANE ONE GENE: E[g][c] and V[g][.] in registers, three float64 accumulators; per list entry m_n, Z_n,
//                    total_n and the U row are wave-uniform (scalar loads), eta and w are recomputed with the cell phase's statements (the same bits) and
//                    p = w / Z (a division: p = 1 exactly where w = Z).  Every term is formed per (cell, gene).  Strip sums go to genepart[strip][3][G].
//   k_predmom_finish a thread per (clone, gene) adds the clone's strips in ascending order onto the call's running tables acc[3][C][G] (zero at the start; the
//                    batches arrive in order): no atomics anywhere, two calls agree bit for bit.

#define CA_PM_TB 256                 // threads per block of all four kernels
#define CA_PM_WAVES (CA_PM_TB / 64)
#define CA_PM_LDS 61440              // dynamic LDS of k_predmom_cell: the row of w up to 7680 genes

struct ca_pm_strip { int32_t lo, cnt, clone; };   // list entries [lo, lo + cnt), all of one clone

__global__ void __launch_bounds__(CA_PM_TB)
k_predmom_loge(const double* __restrict__ Et, double* __restrict__ lEt, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * CA_PM_TB + threadIdx.x;
  if (i < n) {
    const double e = Et[i];
    lEt[i] = e > 0.0 ? log(e) : 0.0;
  }
}

// the block's sum / maximum of v in the fixed order; every thread returns the same value.  x_red: CA_PM_WAVES doubles of LDS, free again on return.
__device__ __forceinline__ double pm_block_sum(double v, double* x_red) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  if ((threadIdx.x & 63) == 0) x_red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = x_red[0];
  for (int k = 1; k < CA_PM_WAVES; ++k) s += x_red[k];
  __syncthreads();
  return s;
}
__device__ __forceinline__ double pm_block_max(double v, double* x_red) {
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
  if ((threadIdx.x & 63) == 0) x_red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = x_red[0];
  for (int k = 1; k < CA_PM_WAVES; ++k) s = fmax(s, x_red[k]);
  __syncthreads();
  return s;
}

// the block's largest v and the lowest index that holds it, in v and i of every thread (max is exact under any grouping).  x_red, x_idx: CA_PM_WAVES entries of LDS.
__device__ __forceinline__ void pm_block_argmax(double& v, int& i, double* x_red, int* x_idx) {
  for (int off = 32; off > 0; off >>= 1) {
    const double ov = __shfl_xor(v, off);
    const int oi = __shfl_xor(i, off);
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
  }
  if ((threadIdx.x & 63) == 0) { x_red[threadIdx.x >> 6] = v; x_idx[threadIdx.x >> 6] = i; }
  __syncthreads();
  v = x_red[0]; i = x_idx[0];
  for (int k = 1; k < CA_PM_WAVES; ++k)
    if (x_red[k] > v || (x_red[k] == v && x_idx[k] < i)) { v = x_red[k]; i = x_idx[k]; }
  __syncthreads();
}

__global__ void __launch_bounds__(CA_PM_TB)
k_predmom_cell(const double* __restrict__ Et /*[C][G]*/, const double* __restrict__ lEt /*[C][G]: log E, 0 where E = 0*/, const double* __restrict__ Vt /*[D][G]*/,
               const double* __restrict__ U /*[cells][D]*/, const int32_t* __restrict__ clone /*[cells]*/, const int64_t* __restrict__ total /*[cells]*/,
               double* w_blk /*[blocks][G], or null: the row is in LDS*/, double* __restrict__ m_out /*[cells]*/, double* __restrict__ z_out /*[cells]*/,
               double* __restrict__ cell_mean /*[cells]*/, double* __restrict__ cell_var /*[cells]*/, int64_t n_cnt, int G, int D) {
  extern __shared__ double pm_sm[];
  __shared__ double x_red[CA_PM_WAVES];
  __shared__ int x_idx[CA_PM_WAVES];
  const int tid = threadIdx.x;
  double* wb = w_blk ? w_blk + (size_t)blockIdx.x * G : pm_sm;
  for (int64_t cell = blockIdx.x; cell < n_cnt; cell += gridDim.x) {
    const int64_t tot = total[cell];
    if (tot == 0) {   // (block-uniform) exactly 0, whatever the clone; the gene phase never lists the cell
      if (tid == 0) { cell_mean[cell] = 0.0; cell_var[cell] = 0.0; m_out[cell] = 0.0; z_out[cell] = 1.0; }
      continue;
    }
    const double* __restrict__ e = Et + (size_t)clone[cell] * G;
    const double* __restrict__ le = lEt + (size_t)clone[cell] * G;
    const double* __restrict__ u = U + cell * D;
    // 1. the shift (k_simulate's step 1)
    double m = -HUGE_VAL;
    for (int g = tid; g < G; g += CA_PM_TB)
      if (e[g] > 0.0) m = fmax(m, sim_eta(u, Vt, D, G, g));
    m = pm_block_max(m, x_red);
    // 2. the weights, the largest of them (the first such gene) and the sum: the others in the fixed order, then the largest
    double acc = 0.0, wmax = -1.0;
    int gmax = G;
    for (int g = tid; g < G; g += CA_PM_TB) {
      const double eg = e[g];
      double w = 0.0;
      if (eg > 0.0) w = eg * exp(__dsub_rn(sim_eta(u, Vt, D, G, g), m));
      wb[g] = w;
      if (w > wmax) { wmax = w; gmax = g; }
    }
    pm_block_argmax(wmax, gmax, x_red, x_idx);   // wmax > 0: the gene at the largest eta has w = E > 0 (the host refused an all-zero clone)
    for (int g = tid; g < G; g += CA_PM_TB)
      if (g != gmax) acc += wb[g];
    const double rest = pm_block_sum(acc, x_red);
    const double Z = rest + wmax;
    const double log_z = log(Z);
    // a gene with p > 1/2: log p = log1p(-(the others' share)), which keeps its relative accuracy where log E + x - log Z cancels; 0 exactly for a lone gene
    const bool top = wmax / Z > 0.5;
    const int gtop = top ? gmax : -1;
    const double lp_top = top ? log1p(-(rest / Z)) : 0.0;
    // 3. h = sum_g p lp
    acc = 0.0;
    for (int g = tid; g < G; g += CA_PM_TB)
      if (e[g] > 0.0) {
        const double lp = g == gtop ? lp_top : le[g] + __dsub_rn(sim_eta(u, Vt, D, G, g), m) - log_z;
        acc += (wb[g] / Z) * lp;
      }
    const double h = pm_block_sum(acc, x_red);
    // 4. the centred variance
    acc = 0.0;
    for (int g = tid; g < G; g += CA_PM_TB)
      if (e[g] > 0.0) {
        const double d = (g == gtop ? lp_top : le[g] + __dsub_rn(sim_eta(u, Vt, D, G, g), m) - log_z) - h;
        acc += (wb[g] / Z) * (d * d);
      }
    const double v = pm_block_sum(acc, x_red);
    if (tid == 0) {
      const double t = (double)tot;
      cell_mean[cell] = t * h; cell_var[cell] = t * v; m_out[cell] = m; z_out[cell] = Z;
    }
  }
}

template <int D>
__global__ void __launch_bounds__(CA_PM_TB)
k_predmom_gene(const double* __restrict__ Et /*[C][G]*/, const double* __restrict__ Vt /*[D][G]*/, const double* __restrict__ U /*[cells][D]*/,
               const int64_t* __restrict__ total /*[cells]*/, const double* __restrict__ m_in /*[cells]*/, const double* __restrict__ z_in /*[cells]*/,
               const int32_t* __restrict__ list /*[live cells], sorted by clone*/, const ca_pm_strip* __restrict__ strips, double* __restrict__ genepart /*[strips][3][G]*/,
               int G, int gtiles) {
  const int tile = blockIdx.x % gtiles, s = blockIdx.x / gtiles;
  const int g = tile * CA_PM_TB + threadIdx.x;
  const bool live = g < G;
  const int gg = live ? g : G - 1;   // (a lane past the last gene works on the last one and stores nothing)
  const ca_pm_strip st = strips[s];
  const double eg = Et[(size_t)st.clone * G + gg];
  double v[D];
#pragma unroll
  for (int d = 0; d < D; ++d) v[d] = Vt[(size_t)d * G + gg];
  double a1 = 0.0, a2 = 0.0, a3 = 0.0;
  for (int i = st.lo; i < st.lo + st.cnt; ++i) {
    const int n = __builtin_amdgcn_readfirstlane(list[i]);
    const double t = (double)total[n], m = m_in[n], Z = z_in[n];
    const double* __restrict__ u = U + (size_t)n * D;
    double eta = __dmul_rn(u[0], v[0]);   // sim_eta's roundings
#pragma unroll
    for (int d = 1; d < D; ++d) eta = __dadd_rn(eta, __dmul_rn(u[d], v[d]));
    double w = 0.0;
    if (eg > 0.0) w = eg * exp(__dsub_rn(eta, m));
    const double p = w / Z, q = 1.0 - p;
    const double tp = t * p, tpq = tp * q;
    a1 += tp;
    a2 += tpq;
    a3 += tpq * (1.0 - 2.0 * p);
  }
  if (live) {
    double* out = genepart + (size_t)s * 3 * G + g;
    out[0] = a1; out[(size_t)G] = a2; out[2 * (size_t)G] = a3;
  }
}

__global__ void __launch_bounds__(CA_PM_TB)
k_predmom_finish(const double* __restrict__ genepart /*[strips][3][G]*/, const int32_t* __restrict__ first /*[C + 1]: clone c owns strips [first[c], first[c + 1])*/,
                 double* __restrict__ acc /*[3][C][G]*/, int G, int C) {
  const int64_t i = (int64_t)blockIdx.x * CA_PM_TB + threadIdx.x, CG = (int64_t)C * G;
  if (i >= CG) return;
  const int c = (int)(i / G), g = (int)(i % G);
  double a1 = acc[i], a2 = acc[CG + i], a3 = acc[2 * CG + i];
  for (int s = first[c]; s < first[c + 1]; ++s) {
    const double* in = genepart + (size_t)s * 3 * G + g;
    a1 += in[0]; a2 += in[(size_t)G]; a3 += in[2 * (size_t)G];
  }
  acc[i] = a1; acc[CG + i] = a2; acc[2 * CG + i] = a3;
}
