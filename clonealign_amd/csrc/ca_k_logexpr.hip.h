// ca_k_logexpr.hip.h -- part of ca_kernels.hip.h (textually included there, in this order): sums of the log-expression lc_ng = log2(y_ng / sf_n + 1) (scater's
// logcounts: size factor of the cell, pseudo-count 1) on the resident count matrix, per gene and cell group (ca_logexpr_sums; the data side of plot_clonealign,
// R/plotting.R:177-205):  S1[g][q] = sum over the cells of group q of lc_ng,  S2[g] = sum over all used cells of lc_ng^2.
//
// One sweep over the [N][Gp] matrix in its own storage (u8 + overflow list, u16, f32), everything in float64; k_fit_mse's walk (ca_k_mse.hip.h).  The host sorts
// the used cells by group (stable) and cuts the list into BLOCK PIECES that never cross a group boundary (ca_lx_blk), so a block's row of partial column sums
// belongs to one group and the per-group sums fall out of which rows of the slab the finishing kernel adds.  Cells labelled -1 are not in the list and are never read.
//
// Shape: block = one gene segment of 64 * VEC columns x one piece of the list, split evenly over the four waves; 16-byte non-temporal loads, two groups of U rows in
// flight.  y / sf is formed as y * (1 / sf) (one rounding apart).  The float64 log2 is a software routine of some tens of fp64 instructions and lc of a
// zero count is exactly 0 (log2(1)).  u16 / f32: log2 sits behind a per-lane branch on y != 0, which a wave skips only where all its 64 lanes hold a zero
// in that column slot.  u8: within a row lc depends on the stored count alone, so each wave tabulates log2(k / sf + 1) in LDS for k up to the largest
// count among its columns of the row -- one evaluation of log2 per 64 table entries instead of one per column slot, none where the piece of the row is
// all zero -- and every slot looks its value up; only 255 (genuine, or an escape to the overflow list) is computed directly.
//
// Reductions, all in a fixed order (no atomics; two calls agree bit for bit):
//   per-lane column sums over the wave's rows (list order) -> the block's four waves ((w0 + w1) + (w2 + w3)) through LDS -> part1 / part2 [piece][Gp] ->
//   k_lx_finish adds, in k_colsum's order, the pieces of one group (S1) or all pieces (S2).
struct ca_lx_blk {    // one block's piece of the sorted list: entries [r0, r0 + nrows), all of one group
  long long r0;
  int nrows, pad;
};

// meta[i] for list entry i = (cell, group): ca_mse_row with a = 1 / size factor and the cell's range of the overflow list
__global__ void __launch_bounds__(CA_TB) k_lx_prep(const int2* __restrict__ list /*[M] (cell, group)*/, const double* __restrict__ inv_sf /*[M], list order*/,
                                                   const int64_t* __restrict__ orowptr /* or null */, ca_mse_row* __restrict__ meta, int64_t M) {
  const int64_t i = (int64_t)blockIdx.x * CA_TB + threadIdx.x;
  if (i >= M) return;
  const int2 e = list[i];
  ca_mse_row m;
  m.n = e.x; m.c = e.y;
  m.a = inv_sf[i];
  m.oe0 = orowptr ? orowptr[e.x] : 0;
  m.noe = orowptr ? (int)(orowptr[e.x + 1] - orowptr[e.x]) : 0;
  m.pad = 0;
  meta[i] = m;
}

template <typename YT>
__global__ void __launch_bounds__(CA_TB) k_logexpr(const YT* __restrict__ Y, const ca_mse_row* __restrict__ meta, const ca_lx_blk* __restrict__ blk /*[nrg]*/,
                                                   const int* __restrict__ ocol, const float* __restrict__ oval, double* __restrict__ part1 /*[nrg][Gp]*/,
                                                   double* __restrict__ part2 /*[nrg][Gp]*/, int G, int Gp, int nseg) {
  constexpr int VEC = YVec<YT>::VEC;
  constexpr int U = CA_MSE_U;
  __shared__ double comb[CA_TB / 64][64 * VEC];
  __shared__ double tab[sizeof(YT) == 1 ? CA_TB / 64 : 1][sizeof(YT) == 1 ? 256 : 1];   // u8: one wave's table of lc by stored count, rebuilt per row
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int rg = (int)blockIdx.x / nseg;   // wave-uniform from here on
  const int sg = (int)blockIdx.x - rg * nseg;
  const ca_lx_blk b = blk[rg];
  const int per = (b.nrows + CA_TB / 64 - 1) / (CA_TB / 64);   // the piece in four runs of `per` entries, one per wave
  const int lo = wave * per;
  const int nrows = (lo < b.nrows) ? ((b.nrows - lo < per) ? b.nrows - lo : per) : 0;
  const int col0 = sg * 64 * VEC + lane * VEC;
  const bool edge = col0 + VEC > G;   // this lane holds padding columns (last segment only)
  const ca_mse_row* __restrict__ mrow = meta + b.r0 + lo;
  const char* base = reinterpret_cast<const char*>(Y) + (int64_t)col0 * (int64_t)sizeof(YT);
  const int64_t pitch = (int64_t)Gp * (int64_t)sizeof(YT);
  double s1[VEC], s2[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) { s1[j] = 0.0; s2[j] = 0.0; }
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
        const double inv = mrow[i].a;
        float y[VEC];
        YVec<YT>::decode(buf[u], y);
        if (edge) {
#pragma unroll
          for (int j = 0; j < VEC; ++j)
            if (col0 + j >= G) y[j] = 0.f;
        }
        if constexpr (sizeof(YT) == 1) {
          // u8: the row's stored counts are 0..255, so lc is a function of the count alone within this row.  The wave tabulates log2(k * inv + 1) for
          // k = 0 .. the largest count of its 64 * VEC columns (64 entries per evaluation of log2: ONE for a row whose counts stay below 64, none for an
          // all-zero piece of a row) and every slot looks its value up; 255 (a genuine 255 or an escape to the overflow list) takes the direct form.
          float mx = 0.f;
#pragma unroll
          for (int j = 0; j < VEC; ++j) mx = fmaxf(mx, y[j]);
#pragma unroll
          for (int o = 1; o < 64; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
          const int top = __builtin_amdgcn_readfirstlane((int)mx);
          if (top > 0) {   // wave-uniform
            const int nt = top < 255 ? top : 254;
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");   // (the lookups of the previous row are done before the table is rewritten)
            for (int k0 = 0; k0 <= nt; k0 += 64) tab[wave][k0 + lane] = log2((double)(k0 + lane) * inv + 1.0);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");   // (one wave writes and reads its own table: LDS keeps a wave's accesses in order)
            const int noe = mrow[i].noe;
            const long long oe0 = mrow[i].oe0;
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
              double lc;
              if (y[j] == 255.f) {   // per lane, rare
                double yd = 255.0;
                if (noe > 0) yd += ca_mse_excess(ocol, oval, oe0, noe, col0 + j);
                lc = log2(yd * inv + 1.0);
              } else {
                lc = tab[wave][(int)y[j]];   // entry 0 is log2(1) = 0 exactly
              }
              s1[j] += lc;
              s2[j] += lc * lc;
            }
          }
        } else {
#pragma unroll
          for (int j = 0; j < VEC; ++j) {
            if (y[j] != 0.f) {   // per lane: a zero count adds exactly 0 to both sums (skipped only where the whole wave holds zeros in this slot)
              const double lc = log2((double)y[j] * inv + 1.0);
              s1[j] += lc;
              s2[j] += lc * lc;
            }
          }
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
  // the four waves' column sums in a fixed order -> the block's rows of part1 and part2
#pragma unroll
  for (int j = 0; j < VEC; ++j) comb[wave][lane * VEC + j] = s1[j];
  __syncthreads();
  for (int i = threadIdx.x; i < 64 * VEC; i += CA_TB)
    part1[(int64_t)rg * Gp + sg * 64 * VEC + i] = (comb[0][i] + comb[1][i]) + (comb[2][i] + comb[3][i]);
  __syncthreads();
#pragma unroll
  for (int j = 0; j < VEC; ++j) comb[wave][lane * VEC + j] = s2[j];
  __syncthreads();
  for (int i = threadIdx.x; i < 64 * VEC; i += CA_TB)
    part2[(int64_t)rg * Gp + sg * 64 * VEC + i] = (comb[0][i] + comb[1][i]) + (comb[2][i] + comb[3][i]);
}

// The finishing sums (k_colsum's shape and order: 64 columns x 16 row lanes, four chains per lane, LDS tree).  blockIdx.y = q < Q: out[q][Gp] = the rows
// [first[q], first[q + 1]) of part1, the pieces of group q (zero for an empty group); blockIdx.y = Q: out[Q][Gp] = all nrg rows of part2.
__global__ void __launch_bounds__(1024) k_lx_finish(const double* __restrict__ part1, const double* __restrict__ part2, const int* __restrict__ first /*[Q + 1]*/,
                                                    int Q, int Gp, double* __restrict__ out /*[Q + 1][Gp]*/) {
  constexpr int RL = 16;
  __shared__ double sm[RL][64];
  const int q = blockIdx.y;
  const double* __restrict__ src = q < Q ? part1 : part2;
  const int r_lo = q < Q ? first[q] : 0, r_hi = q < Q ? first[q + 1] : first[Q];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + tx;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  if (c < Gp) {
    int r = r_lo + ty;
    for (; r + 3 * RL < r_hi; r += 4 * RL) {
      a0 += src[(int64_t)r * Gp + c]; a1 += src[(int64_t)(r + RL) * Gp + c];
      a2 += src[(int64_t)(r + 2 * RL) * Gp + c]; a3 += src[(int64_t)(r + 3 * RL) * Gp + c];
    }
    for (; r < r_hi; r += RL) a0 += src[(int64_t)r * Gp + c];
    a0 += a2; a1 += a3;
  }
  sm[ty][tx] = a0 + a1;
  __syncthreads();
#pragma unroll
  for (int s = RL / 2; s > 0; s >>= 1) {
    if (ty < s) sm[ty][tx] += sm[ty + s][tx];
    __syncthreads();
  }
  if (ty == 0 && c < Gp) out[(int64_t)q * Gp + c] = sm[0][tx];
}
