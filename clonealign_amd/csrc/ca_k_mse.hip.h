// ca_k_mse.hip.h -- part of ca_kernels.hip.h (textually included there, in this order): the squared error of a fit on the resident count matrix (ca_fit_mse;
// compute_ca_fit_mse, R/clonealign.R:415-434): r_ng = a_n E[g][c_n] - y_ng, a_n = rowsum_n / sum_g E[g][c_n], summed as r^2 per gene, per cell and in total.
//
// One sweep over the [N][Gp] matrix in its own storage (u8 + overflow list, u16, f32), everything in float64: the residual is formed and squared per count.
// The table E is G x C doubles (320 KB at 5000 x 8): it is never staged whole.  The host sorts the used cells by clone (stable), so a wave walks a strip of TR
// list entries that almost always share one clone and keeps that clone's VEC values of E for its own columns in registers (GATHER BY CLONE: a reload of
// 8 * VEC bytes per lane from L2 where the clone changes, nothing per count).  Cells labelled -1 are not in the list and are never read.
//
// Shape: the vector stream's (k_ypass): block = one gene segment of 64 * VEC columns x four strips (one per wave), 16-byte non-temporal loads, two groups of U
// rows in flight.  A lane spends about five fp64 instructions per count (convert, a e - y, square, two adds): at 16 fp64 lanes per SIMD and clock a u8 row
// takes about as long to compute as HBM takes to deliver it, and the u8 instantiation holds 202 VGPRs (two waves per SIMD) -- DESIGN.md section 7.
//
// Reductions, all in a fixed order (no atomics; two calls agree bit for bit):
//   cell:  lane sum over its VEC columns (ascending) -> xor butterfly over the wave -> cellpart[segment][list entry] -> k_mse_finish adds the segments ascending
//   gene:  per-lane column sums over the strip's rows (list order) -> the block's four waves ((w0 + w1) + (w2 + w3)) -> genepart[row group][Gp] ->
//          k_mse_finish adds the row groups in k_colsum's order
// The per-cell sum does not depend on the strip length or on the cell's place in the list, so a cell-sharded group returns the single handle's bits.
struct ca_mse_row {   // one used cell, in list order (made by k_mse_prep)
  int n, c;           // cell, clone
  double a;           // rowsum_n / sum_g E[g][c]
  long long oe0;      // u8 storage: the cell's range of the overflow list (CSR copy)
  int noe, pad;
};

__global__ void __launch_bounds__(CA_TB) k_mse_prep(const int2* __restrict__ list /*[M] (cell, clone)*/, const double* __restrict__ s64, const double* __restrict__ esum /*[C]*/,
                                                    const int64_t* __restrict__ orowptr /* or null */, ca_mse_row* __restrict__ meta, int64_t M) {
  const int64_t i = (int64_t)blockIdx.x * CA_TB + threadIdx.x;
  if (i >= M) return;
  const int2 e = list[i];
  ca_mse_row m;
  m.n = e.x; m.c = e.y;
  m.a = s64[e.x] / esum[e.y];
  m.oe0 = orowptr ? orowptr[e.x] : 0;
  m.noe = orowptr ? (int)(orowptr[e.x + 1] - orowptr[e.x]) : 0;
  m.pad = 0;
  meta[i] = m;
}

// the excess over 255 of count (cell, g) from the cell's sorted range of the overflow list; 0 when the count is a genuine 255
__device__ __forceinline__ double ca_mse_excess(const int* __restrict__ ocol, const float* __restrict__ oval, long long oe0, int noe, int g) {
  int lo = 0, hi = noe;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ocol[oe0 + mid] < g) lo = mid + 1; else hi = mid;
  }
  return (lo < noe && ocol[oe0 + lo] == g) ? (double)oval[oe0 + lo] : 0.0;
}

#ifndef CA_MSE_U
#define CA_MSE_U 4   // rows per group; two groups alternate
#endif
template <typename YT>
__global__ void __launch_bounds__(CA_TB) k_fit_mse(const YT* __restrict__ Y, const ca_mse_row* __restrict__ meta, const double* __restrict__ Et /*[C][Gp], zero padded*/,
                                                   const int* __restrict__ ocol, const float* __restrict__ oval, double* __restrict__ cellpart /*[nseg][M]*/,
                                                   double* __restrict__ genepart /*[nrg][Gp]*/, int64_t M, int G, int Gp, int nseg, int nrb, int TR) {
  constexpr int VEC = YVec<YT>::VEC;
  constexpr int U = CA_MSE_U;
  __shared__ double comb[CA_TB / 64][64 * VEC];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int rg = (int)blockIdx.x / nseg;   // wave-uniform from here on
  const int sg = (int)blockIdx.x - rg * nseg;
  const int rb = rg * (CA_TB / 64) + wave;
  const bool live = rb < nrb;
  const int col0 = sg * 64 * VEC + lane * VEC;
  const bool edge = col0 + VEC > G;   // this lane holds padding columns (last segment only)
  const int64_t r0 = live ? (int64_t)rb * TR : 0;
  const int nrows = live ? (int)(((r0 + TR < M) ? r0 + TR : M) - r0) : 0;
  const ca_mse_row* __restrict__ mrow = meta + r0;
  const char* base = reinterpret_cast<const char*>(Y) + (int64_t)col0 * (int64_t)sizeof(YT);
  const int64_t pitch = (int64_t)Gp * (int64_t)sizeof(YT);
  double e[VEC], acc[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) { e[j] = 0.0; acc[j] = 0.0; }
  int cur_c = -1;
  double keep = 0.0;
  auto fetch = [&](uint4 (&buf)[U], int i0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = (i0 + u < nrows) ? i0 + u : nrows - 1;   // tail rows re-read the last row (never consumed)
      const int64_t n = mrow[i].n;
      typedef unsigned v4u_ __attribute__((ext_vector_type(4)));   // streamed once: non-temporal, like the loop's stream
      const v4u_ t_ = __builtin_nontemporal_load(reinterpret_cast<const v4u_*>(base + n * pitch));
      buf[u] = (uint4){t_.x, t_.y, t_.z, t_.w};
    }
  };
  auto consume = [&](const uint4 (&buf)[U], int i0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = i0 + u;
      if (i < nrows) {   // wave-uniform
        const int c = mrow[i].c;
        const double a = mrow[i].a;
        if (c != cur_c) {   // wave-uniform: the list is sorted by clone
          cur_c = c;
          const double* ep = Et + (int64_t)c * Gp + col0;
#pragma unroll
          for (int j = 0; j < VEC; ++j) e[j] = ep[j];
        }
        float y[VEC];
        YVec<YT>::decode(buf[u], y);
        if (edge) {
#pragma unroll
          for (int j = 0; j < VEC; ++j)
            if (col0 + j >= G) y[j] = 0.f;
        }
        double yd[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) yd[j] = (double)y[j];
        if constexpr (sizeof(YT) == 1) {
          const int noe = mrow[i].noe;
          if (noe > 0) {   // wave-uniform: this cell has counts above 255, stored as 255 + an entry of the list
            const long long oe0 = mrow[i].oe0;
#pragma unroll
            for (int j = 0; j < VEC; ++j)
              if (y[j] == 255.f) yd[j] += ca_mse_excess(ocol, oval, oe0, noe, col0 + j);
          }
        }
        double rs = 0.0;
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          const double r = a * e[j] - yd[j];
          const double q = r * r;
          acc[j] += q;
          rs += q;
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) rs += __shfl_xor(rs, o, 64);
        if (lane == (i & 63)) keep = rs;
        if ((i & 63) == 63 || i == nrows - 1) {   // wave-uniform flush of the last (up to 64) row sums
          const int fb = i & ~63;
          if (fb + lane <= i) cellpart[(int64_t)sg * M + r0 + fb + lane] = keep;
        }
      }
    }
  };
  uint4 bufA[U], bufB[U];
  if (nrows > 0) fetch(bufA, 0);
  for (int i0 = 0; i0 < nrows; i0 += 2 * U) {
    if (i0 + U < nrows) fetch(bufB, i0 + U);
    consume(bufA, i0);
    if (i0 + 2 * U < nrows) fetch(bufA, i0 + 2 * U);
    if (i0 + U < nrows) consume(bufB, i0 + U);
  }
  // the four waves' column sums in a fixed order -> the block's row of genepart
#pragma unroll
  for (int j = 0; j < VEC; ++j) comb[wave][lane * VEC + j] = acc[j];
  __syncthreads();
  for (int i = threadIdx.x; i < 64 * VEC; i += CA_TB)
    genepart[(int64_t)rg * Gp + sg * 64 * VEC + i] = (comb[0][i] + comb[1][i]) + (comb[2][i] + comb[3][i]);
}

// The finishing sums: blocks [0, nb_gene) add genepart's row groups per gene (k_colsum's shape and order: 64 columns x 16 row lanes, four chains per lane, LDS
// tree), the blocks behind them add cellpart's segments per list entry and scatter the sum to its cell (sse_cell is zero elsewhere: skipped cells).
__global__ void __launch_bounds__(1024) k_mse_finish(const double* __restrict__ genepart, int nrg, int Gp, double* __restrict__ sse_gene /*[Gp]*/,
                                                     const double* __restrict__ cellpart, const ca_mse_row* __restrict__ meta, int64_t M, int nseg,
                                                     double* __restrict__ sse_cell /*[N]*/, int nb_gene) {
  constexpr int RL = 16;
  __shared__ double sm[RL][64];
  if ((int)blockIdx.x >= nb_gene) {
    const int64_t i = (int64_t)((int)blockIdx.x - nb_gene) * 1024 + threadIdx.x;
    if (i < M) {
      double s = 0.0;
      for (int sg = 0; sg < nseg; ++sg) s += cellpart[(int64_t)sg * M + i];
      sse_cell[meta[i].n] = s;
    }
    return;
  }
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + tx;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  if (c < Gp) {
    int r = ty;
    for (; r + 3 * RL < nrg; r += 4 * RL) {
      a0 += genepart[(int64_t)r * Gp + c]; a1 += genepart[(int64_t)(r + RL) * Gp + c];
      a2 += genepart[(int64_t)(r + 2 * RL) * Gp + c]; a3 += genepart[(int64_t)(r + 3 * RL) * Gp + c];
    }
    for (; r < nrg; r += RL) a0 += genepart[(int64_t)r * Gp + c];
    a0 += a2; a1 += a3;
  }
  sm[ty][tx] = a0 + a1;
  __syncthreads();
#pragma unroll
  for (int s = RL / 2; s > 0; s >>= 1) {
    if (ty < s) sm[ty][tx] += sm[ty + s][tx];
    __syncthreads();
  }
  if (ty == 0 && c < Gp) sse_gene[c] = sm[0][tx];
}
