// ca_k_cnprofile.hip.h -- part of ca_kernels.hip.h (textually included there, after ca_k_separability.hip.h): the device side of the copy-number likelihood
// profile (ca_copy_number_profile; include/clonealign_hip.h states the output).  Replacing the weight E[g][c] by mu_g kappa_j for the genes of one block, in clone
// c only, changes a cell's -log Z by -log1p(sum_{g in block} (mu_g kappa_j - E[g][c]) x_ng), x_ng = exp(eta_ng - m_n) / Z_n; the kernels sum total_n log1p(.)
// over a clone's cells per (block-or-gene, candidate).  No count matrix is read.  D > 0 only (without factors x depends on the clone alone: the host's work).
//   k_cnp_cell    A BLOCK OWNS A CELL (k_predmom_cell's walk): m_n and Z_n by that kernel's steps 1 and 2, statement for statement -- the same bits.  In block
//                 mode a third pass: a WAVE owns a block of genes (the host's run list: the genes stably sorted by label), a lane the run's entries lane, lane
//                 + 64, ... ascending, the wave's sum by the xor butterfly: A[n][b] = sum mu_g x_ng and S[n][b] = sum p_ng (p = w / Z, k_predmom_gene's p), a fixed
//                 order for any labelling.  S = 1 exactly where the block holds every expressed gene of the cell's clone (the host's table `full`), at most 1 - 2^-53 elsewhere.
//   k_cnp_gene    per-gene mode, the hot path, k_predmom_gene's shape: a BLOCK OWNS 256 GENES x ONE STRIP of the list (cells with total > 0 by clone), A LANE ONE
//                 GENE.  In registers: E[g][c], the gene's V row and JB coefficients cf_j = (mu_g kappa_j - E) / E (E > 0; mu_g kappa_j where E = 0; the products
//                 come rounded from the host, so that mu_g kappa_j == E gives 0 exactly), unused slots 0;
//                 JB float64 accumulators indexed at compile time (JB = 4, 8, 16: one instantiation each; D is a run-time bound on an unrolled loop, so V's row
//                 is a register array all the same).  Per list entry m, Z, total and the U row are wave-uniform; one exp and one division per (cell, gene): q = p
//                 = w / Z where E > 0 (1 exactly where w = Z), exp(eta - m) / Z where E = 0; then a_j = cf_j q >= -1 and JB log1p.  cf_j = 0 gives exactly 0.
//   k_cnp_block   block mode: a lane per (candidate, block) runs over a strip's entries: a = max(kappa_j A - S, -1), total log1p(a); 0 by rule where the host's
//                 table says that every gene of the block has mu_g kappa_j == E[g][c] bit for bit.
//   k_cnp_finish  a thread per (clone, candidate, block-or-gene) adds the clone's strips in ascending order onto the running table acc[C][J][W]: no atomics.

#define CA_CNP_SMAX 0x1.fffffffffffffp-1   // 1 - 2^-53, the largest share S of a block that does not hold every expressed gene of the cell's clone

template <int JB>
__global__ void __launch_bounds__(CA_PM_TB)
k_cnp_gene(const double* __restrict__ Et /*[C][G]*/, const double* __restrict__ Vt /*[D][G]*/, const double* __restrict__ U /*[cells][D]*/,
           const int64_t* __restrict__ total /*[cells]*/, const double* __restrict__ m_in /*[cells]*/, const double* __restrict__ z_in /*[cells]*/,
           const int32_t* __restrict__ list /*[live cells], sorted by clone*/, const ca_pm_strip* __restrict__ strips,
           const double* __restrict__ mk /*[J][G]: mu_g kappa_j, rounded on the host*/, double* __restrict__ part /*[strips][J][G]*/, int G, int D, int J, int gtiles) {
  const int tile = blockIdx.x % gtiles, s = blockIdx.x / gtiles;
  const int g = tile * CA_PM_TB + threadIdx.x;
  const bool live = g < G;
  const int gg = live ? g : G - 1;   // (a lane past the last gene works on the last one and stores nothing)
  const ca_pm_strip st = strips[s];
  const double eg = Et[(size_t)st.clone * G + gg];
  const bool pos = eg > 0.0;
  double v[CA_LL_DMAX], cf[JB], acc[JB];
#pragma unroll
  for (int d = 0; d < CA_LL_DMAX; ++d) v[d] = d < D ? Vt[(size_t)d * G + gg] : 0.0;
#pragma unroll
  for (int j = 0; j < JB; ++j) {
    double c = 0.0;
    if (j < J) {
      const double dl = mk[(size_t)j * G + gg] - eg;   // (the product is a load: the device's a * b - c would be one fused operation, never 0 for an inexact product)
      c = pos ? dl / eg : dl;
    }
    cf[j] = c; acc[j] = 0.0;
  }
  for (int i = st.lo; i < st.lo + st.cnt; ++i) {
    const int n = __builtin_amdgcn_readfirstlane(list[i]);
    const double t = (double)total[n], m = m_in[n], Z = z_in[n];
    const double* __restrict__ u = U + (size_t)n * D;
    double eta = __dmul_rn(u[0], v[0]);   // sim_eta's roundings
#pragma unroll
    for (int d = 1; d < CA_LL_DMAX; ++d)
      if (d < D) eta = __dadd_rn(eta, __dmul_rn(u[d], v[d]));
    const double ex = exp(__dsub_rn(eta, m));
    const double q = (pos ? eg * ex : ex) / Z;   // E > 0: p = w / Z, the cell phase's w
#pragma unroll
    for (int j = 0; j < JB; ++j) {
      const double a = cf[j] == 0.0 ? 0.0 : cf[j] * q;
      acc[j] += t * log1p(a);
    }
  }
  if (live) {
#pragma unroll
    for (int j = 0; j < JB; ++j)
      if (j < J) part[((size_t)s * J + j) * G + g] = acc[j];
  }
}

__global__ void __launch_bounds__(CA_PM_TB)
k_cnp_cell(const double* __restrict__ Et /*[C][G]*/, const double* __restrict__ Vt /*[D][G]*/, const double* __restrict__ U /*[cells][D]*/,
           const int32_t* __restrict__ clone /*[cells]*/, const int64_t* __restrict__ total /*[cells]*/, double* w_blk /*[blocks][G], or null: the row is in LDS*/,
           double* __restrict__ m_out /*[cells]*/, double* __restrict__ z_out /*[cells]*/, const double* __restrict__ mu /*[G]*/,
           const int32_t* __restrict__ run_gene /*[G]: the genes by block, or null: per-gene mode*/, const int32_t* __restrict__ run_first /*[B + 1]*/,
           const unsigned char* __restrict__ full /*[C][B]*/, double* __restrict__ share /*[cells][2][B]: A, S*/, int64_t n_cnt, int G, int D, int B) {
  extern __shared__ double pm_sm[];
  __shared__ double x_red[CA_PM_WAVES];
  __shared__ int x_idx[CA_PM_WAVES];
  const int tid = threadIdx.x;
  double* wb = w_blk ? w_blk + (size_t)blockIdx.x * G : pm_sm;
  for (int64_t cell = blockIdx.x; cell < n_cnt; cell += gridDim.x) {
    if (total[cell] == 0) {   // (block-uniform) the gene phase never lists the cell
      if (tid == 0) { m_out[cell] = 0.0; z_out[cell] = 1.0; }
      continue;
    }
    const int c = clone[cell];
    const double* __restrict__ e = Et + (size_t)c * G;
    const double* __restrict__ u = U + cell * D;
    // 1. the shift, 2. the weights, the largest of them and Z = (the others' sum) + the largest: k_predmom_cell's statements
    double m = -HUGE_VAL;
    for (int g = tid; g < G; g += CA_PM_TB)
      if (e[g] > 0.0) m = fmax(m, sim_eta(u, Vt, D, G, g));
    m = pm_block_max(m, x_red);
    double acc = 0.0, wmax = -1.0;
    int gmax = G;
    for (int g = tid; g < G; g += CA_PM_TB) {
      const double eg = e[g];
      double w = 0.0;
      if (eg > 0.0) w = eg * exp(__dsub_rn(sim_eta(u, Vt, D, G, g), m));
      wb[g] = w;
      if (w > wmax) { wmax = w; gmax = g; }
    }
    pm_block_argmax(wmax, gmax, x_red, x_idx);
    for (int g = tid; g < G; g += CA_PM_TB)
      if (g != gmax) acc += wb[g];
    const double rest = pm_block_sum(acc, x_red);
    const double Z = rest + wmax;
    if (tid == 0) { m_out[cell] = m; z_out[cell] = Z; }
    if (!run_gene) continue;
    // 3. the shares of every block of genes: a wave per block, the weights recomputed (a lane reads no other lane's row entries)
    const int lane = tid & 63;
    for (int b = tid >> 6; b < B; b += CA_PM_WAVES) {
      double sa = 0.0, ss = 0.0;
      for (int i = run_first[b] + lane; i < run_first[b + 1]; i += 64) {
        const int g = run_gene[i];
        const double eg = e[g], ex = exp(__dsub_rn(sim_eta(u, Vt, D, G, g), m));
        sa += mu[g] * (ex / Z);
        if (eg > 0.0) ss += (eg * ex) / Z;
      }
      for (int off = 32; off > 0; off >>= 1) { sa += __shfl_xor(sa, off); ss += __shfl_xor(ss, off); }
      if (lane == 0) {
        double* out = share + (size_t)cell * 2 * B;
        out[b] = sa;
        out[B + b] = full[(size_t)c * B + b] ? 1.0 : fmin(ss, CA_CNP_SMAX);   // (below 1 without the rule: a = -1, so -inf, by the rule alone)
      }
    }
  }
}

__global__ void __launch_bounds__(CA_PM_TB)
k_cnp_block(const double* __restrict__ share /*[cells][2][B]*/, const int64_t* __restrict__ total /*[cells]*/, const int32_t* __restrict__ list,
            const ca_pm_strip* __restrict__ strips, const double* __restrict__ kappa /*[J]*/, const unsigned char* __restrict__ same /*[C][J][B]*/,
            double* __restrict__ part /*[strips][J][B]*/, int B, int J, int tiles) {
  const int tile = blockIdx.x % tiles, s = blockIdx.x / tiles;
  const int i = tile * CA_PM_TB + threadIdx.x, JB = J * B;
  const bool live = i < JB;
  const int ii = live ? i : JB - 1;
  const int j = ii / B, b = ii % B;
  const ca_pm_strip st = strips[s];
  const double k = kappa[j];
  const bool zero = same[(size_t)st.clone * JB + ii] != 0;
  double acc = 0.0;
  for (int e = st.lo; e < st.lo + st.cnt; ++e) {
    const int n = __builtin_amdgcn_readfirstlane(list[e]);
    const double t = (double)total[n];
    const double* __restrict__ sh = share + (size_t)n * 2 * B;
    const double a = fmax(__dsub_rn(__dmul_rn(k, sh[b]), sh[B + b]), -1.0);
    acc += t * log1p(a);
  }
  if (live) part[(size_t)s * JB + i] = zero ? 0.0 : acc;
}

__global__ void __launch_bounds__(CA_PM_TB)
k_cnp_finish(const double* __restrict__ part /*[strips][J][W]*/, const int32_t* __restrict__ first /*[C + 1]: clone c owns strips [first[c], first[c + 1])*/,
             double* __restrict__ acc /*[C][J][W]*/, int64_t JW, int C) {
  const int64_t i = (int64_t)blockIdx.x * CA_PM_TB + threadIdx.x;
  if (i >= JW * C) return;
  const int c = (int)(i / JW);
  const int64_t r = i % JW;
  double a = acc[i];
  for (int s = first[c]; s < first[c + 1]; ++s) a += part[(size_t)s * JW + r];
  acc[i] = a;
}
