// ca_poly.hip -- the cells x genes x clones reduction WITHOUT the cells x genes sweep, for a rank-one exponent (K + P = 1, one MC sample).
//
// What the reference computes (R/inference-tflow.R:278-292): E_ng = exp(psi_n W_g), Z_nc = sum_g E_ng mu_g L_gc -- N G C multiply-adds and
// N G exponentials per pass, and as many again on the way back (autodiff of :288-296).  With ONE latent dimension the exponent is a product
// x_n v_g of a per-cell and a per-gene number, and  Z_nc = sum_g M_gc exp(x_n v_g)  is, for every clone, ONE function of x evaluated at N
// points.  Cut the genes into bins by v (width delta, centres v_b) and expand each bin's share around its centre:
//     Z_nc = sum_b exp(x_n v_b) sum_k x_n^k B[b][k][c],     B[b][k][c] = sum_{g in bin b} M_gc (v_g - v_b)^k / k!
// -- a Taylor series of exp(x (v - v_b)) whose argument is bounded by |x|max delta / 2 <= 2 by the choice of delta, so twenty terms leave a
// remainder below 1e-11 relative, in float64, with no cancellation to speak of (e^2 against e^-2).  The moments B cost G R C operations, the
// evaluation N nb R C: the sweep's N G C is gone.  The way back has the same form.  With coef_nc = -gamma_nc s_n / Z_nc (the cell epilogue's,
// unchanged):
//     d ELBO / d mu_g = sum_c L_gc q_c(v_g),   d / d V_g = mu_g sum_c L_gc q_c'(v_g),   q_c(v) = sum_n coef_nc exp(x_n v)
//     q_c(v) = sum_k (v - v_b)^k / k!  Q[b][k][c]  for v in bin b,     Q[b][k][c] = sum_n coef_nc x_n^k exp(x_n v_b)        (all cells, every bin)
//     d / d F_n = sum_c coef_nc dZ_nc / dx                                                                                  (with the forward pass)
// Everything that is not this contraction -- the multinomial log-likelihood, softmax, ELBO partials, coef, d logits: the cell epilogue
// ca_cell_fused_group -- is the code the matrix-core sweep feeds, called with these Z values.  The matrix-core sweeps (ca_kernels.hip.h) remain the
// general path: two or more exponent dimensions, several MC samples, more than eight clones, or an exponent range this expansion would need more
// than CA_PL_NB bins for (the header word `bad`, surfaced as CA_ERR_STATE).  DESIGN.md section 5e.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <type_traits>

#include "ca_poly.h"

namespace ca_series {   // (a namespace of its own: the header's kernels get names that do not clash with the engine unit's, and profiles read "ca_series::k_poly_cell")
#include "ca_kernels.hip.h"   // the cell epilogue and its helpers (this unit instantiates only what it launches)

constexpr int R = CA_PL_R, NB = CA_PL_NB;
#include "ca_polymom.hip.h"     // the moments' bodies: one copy of the arithmetic for these kernels and for the stream launch's moment role
constexpr int TB_B = 384;       // k_poly_B block: one thread per (k, column) output (21 x 16 = 336)
constexpr int GPB = CA_PM_GPB;  // genes per k_poly_B block

__device__ __forceinline__ float warp_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float warp_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}

// ---- K0: max |x| over the cells (an order-preserving unsigned maximum: exact whatever the order); k_poly_red resets the word behind its reader ------------
__global__ void __launch_bounds__(CA_TB) k_poly_xmax(const float* __restrict__ F, int64_t N, unsigned int* __restrict__ xbits) {
  __shared__ float sx[CA_TB / 64];
  float ax = 0.f;
  const int64_t n4 = N / 4;
  const float4* F4 = reinterpret_cast<const float4*>(F);
  for (int64_t i = (int64_t)blockIdx.x * CA_TB + threadIdx.x; i < n4; i += (int64_t)gridDim.x * CA_TB) {
    const float4 v = F4[i];
    ax = fmaxf(fmaxf(ax, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
  }
  if (blockIdx.x == 0 && threadIdx.x < (int)(N - n4 * 4)) ax = fmaxf(ax, fabsf(F[n4 * 4 + threadIdx.x]));
  ax = warp_max(ax);
  if ((threadIdx.x & 63) == 0) sx[threadIdx.x >> 6] = ax;
  __syncthreads();
  if (threadIdx.x == 0) {
    ax = fmaxf(fmaxf(sx[0], sx[1]), fmaxf(sx[2], sx[3]));
    if (!(ax == ax)) ax = INFINITY;                      // (a NaN latent position: the header's `bad` says so)
    atomicMax(xbits, __float_as_uint(ax));               // non-negative floats order like their bit patterns
  }
}

// ---- ranges only: one block scans V, takes the cells' maximum from k_poly_xmax's word (and resets it), mirrors both to the host -------------------------
// (xglob / nglob / xadd: a cell-sharded fit -- max |x| over ALL ranks' cells as the last collective left it, one slot per rank, for the state one Adam step back,
//  plus what that step can have added: the same number on every rank, so that every rank takes the same decisions; see ca_poly_xslot)
__global__ void __launch_bounds__(CA_TB) k_poly_ranges(const float* __restrict__ V, int G, unsigned int* __restrict__ xbits, double* __restrict__ mirror, double seq,
                                                       const float* __restrict__ xpart, int nx, const double* __restrict__ xglob, int nglob, double xadd) {
  __shared__ float smn[CA_TB / 64], smx[CA_TB / 64], sxm[CA_TB / 64];
  const int t = threadIdx.x;
  float mn = INFINITY, mx = -INFINITY;
  float xm = 0.f;   // (nx > 0: max |x| per piece of cells as the merged update left it)
  for (int i = t; i < nx; i += CA_TB) xm = fmaxf(xm, xpart[i]);
  xm = warp_max(xm);
  if ((t & 63) == 0) sxm[t >> 6] = xm;
  constexpr int U = 8;
  for (int g0_ = 0; g0_ < G; g0_ += CA_TB * U) {
    float v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) { const int g = g0_ + u * CA_TB + t; v[u] = V[g < G ? g : G - 1]; }
#pragma unroll
    for (int u = 0; u < U; ++u) { mn = fminf(mn, v[u]); mx = fmaxf(mx, v[u]); }
  }
  mn = warp_min(mn); mx = warp_max(mx);
  if ((t & 63) == 0) { smn[t >> 6] = mn; smx[t >> 6] = mx; }
  __syncthreads();
  if (t == 0) {
    mn = fminf(fminf(smn[0], smn[1]), fminf(smn[2], smn[3]));
    mx = fmaxf(fmaxf(smx[0], smx[1]), fmaxf(smx[2], smx[3]));
    double xmax = nx > 0 ? (double)fmaxf(fmaxf(sxm[0], sxm[1]), fmaxf(sxm[2], sxm[3])) : (double)__uint_as_float(*xbits);
    if (nglob > 0) { xmax = 0.0; for (int r = 0; r < nglob; ++r) xmax = fmax(xmax, xglob[r]); xmax += xadd; }
    *xbits = 0u;
    ca_poly_mirror_store(mirror, seq, xmax, (double)mn, (double)mx);
  }
}

// ---- K1: bin geometry and the forward moments: the body is ca_pm_B_body (ca_polymom.hip.h), shared with the moment role of the count-matrix stream's launch ----
// part[blk][b][k][col] block partials (the 1 / k! inside the powers), summed in block order by k_poly_red into tabB[b][k][col].
// col: draw A clones 0..7 | draw B clones 0..7.  (As launches of their own the blocks share nothing: the kernel boundary hands the partials to the reduction.)
__global__ void __launch_bounds__(TB_B) k_poly_B(ca_pm_args a) {
  __shared__ ca_pm_lds s;
  ca_pm_B_body<TB_B, false>(a, (int)blockIdx.x, 1, blockIdx.x == 0, s);
}

// ---- K2: per cell: Z for both draws and dZ/dx for the train draw by Horner over the bins, the cell epilogue, d/dF, the backward moments --------------
// A block's pass over its 32 (CP = 8) or 64 cells is ONE chain of latencies (two blocks per CU at 241 VGPRs: nothing else on the SIMD to fill it), so what a pass
// costs is the number of round trips on that chain, not its arithmetic.  LEAN (CA_VAR_CELL_LEAN, the default) takes out those the result does not need:
//   * no global load inside a pass but load_pass's prefetch of the NEXT pass -- the exponent bound the epilogue would read is a vector of zeros here, c_n travels
//     with the prefetch, psi of the prior term is x (ca_cell_pre_lean); without them no s_waitcnt vmcnt(0) stands between the loop header and the first barrier,
//     which on this ISA would also wait for the pass's own coef / d logits / dF stores;
//   * the reductions over a cell's 4 or 8 lanes (two maxima / sums of the softmax, the epilogue's f-bar, d/dF) through DPP moves instead of ds_bpermute: twelve
//     dependent trips through the LDS crossbar less per pass (ca_dpp_gsum / ca_dpp_gmax: __shfl_xor's pairing);
//   * the powers x^k by selects into the (up to) RQ / CP values a lane keeps and unconditional stores, instead of 22 steps of "multiply, branch on exec, store".
// Every sum keeps its operands and its order: LEAN = false is the launch as it was, and the two agree to the bit (tests/test_gpu_cell_lean.py).
//
// MFMA (CA_VAR_CELL_MFMA, the default; independent of LEAN) is how the backward moments of the register bins 0 .. NBR - 1 are gathered.  What the gather computes,
//     Q[b][k][c] += sum_{s in pass} x_s^k (coef_sc exp(x_s v_b)),
// is a matrix product with M = k (RQ rows), N = (bin, clone) and the pass's cells as its inner dimension, and everything it reads a wave wrote itself: the wave owns
// 64 / CP of the pass's cells and leaves s_xp, s_cf and s_eb for exactly those.  So each wave multiplies its own cells by v_mfma_f64_16x16x4_f64 -- four cells a step;
// A[row = lane & 15][cell = lane >> 4] = x^k, B[cell = lane >> 4][column = lane & 15] = coef e_b with column = (bin in tile) CP + clone; two row tiles for k = 0 .. 15
// and 16 .. RQ - 1, NBR CP / 16 column tiles -- into accumulators it keeps over all the block's passes; C/D[row = (lane >> 4) + 4 reg][column = lane & 15].  Nothing in
// a pass then crosses a wave, and the two block barriers of the pass give way to wave barriers.  At the block's end the four waves' tiles are added in wave order
// 0, 1, 2, 3 through LDS (the passes' own arrays, idle by then) into the block's slab: layout and meaning as before; the order inside an MFMA is the hardware's
// and every other order is the code's, so the sums are the same from run to run, but not the thread-owned chain's association: fp64 rounding apart.  Bins past NBR
// (a wide exponent range) keep that chain through the slab, and with it the pass's two barriers, under a uniform test.  MFMA = false is the launch as it was.
//
// EDGE (CA_VAR_CELL_EDGE, the default; with LEAN and MFMA only) is what stands around the passes.  The head made three dependent trips to memory -- the bin count,
// then the tables it bounds, then, behind the barrier, the first prefetch -- with the last wave's log softmax(alpha) (twelve crossbar trips, an exp and a log in
// fp64) in front of that barrier.  None needs another's result: the workspace always holds NB tables and those past nb are never read, so alpha, the header, the
// first prefetch and the tables of all NBL bins are issued before the first wait; every wave makes its own copy of log alpha in its own words of la[] through the
// DPP network (xor 1, 2, 4 as the 64-lane butterfly starts; its later steps add an exact 0.0 or compare with -inf).  The block's end took five barrier-separated
// stages; here every wave leaves its three sums (ca_dpp_wave_sum: the butterfly's pairs) and its gamma sums in words the passes never use, one barrier says that
// the passes' arrays are idle, waves 1 - 3 park their tiles, and behind a second barrier wave 0 adds the tiles while wave 1 makes the block sums, each chain's
// loads issued before its adds.  In a pass, the q(z) half of the epilogue (ca_cell_qz_half: it needs the prefetched logit alone) stands with bin 0, peeled out of
// the bins' loop (nb >= 1), where it runs beside that bin's exp and Horner chains instead of behind the loop.  The same operands in the same order: EDGE = false
// is the launch as it was, and the two agree to the bit (tests/test_gpu_cell_edge.py).
template <int CP, bool LEAN, bool MFMA, bool EDGE = false>
__global__ void __launch_bounds__(CA_TB) k_poly_cell(const ca_poly_hdr* __restrict__ hdr, const double* __restrict__ tabB, ca_cell_ptrs p,
                                                     const float* __restrict__ alpha_u, double* __restrict__ cell_part, int64_t N, int C, int K,
                                                     float* __restrict__ dF /*[N]*/, double* __restrict__ Qpart /*[grid][nb][R+2][C]*/, int ncb, ca_yfin_args yfin) {
  // Blocks behind the ncb cell blocks finish the count-matrix stream's products (what k_yfinish does as a launch of its own, 5.4 us and a launch gap on the
  // iteration's critical path): nothing in this launch reads them.  They are this kernel with this kernel's registers (207 - 241 VGPRs: two blocks per CU, and the
  // cell blocks are two to a CU), so none of them runs BESIDE a cell block: each starts in a slot a cell block has left.  The row jobs (YW and the psi.(YW)
  // partials, which the launch that follows reads) are one round of loads and a block sum, short enough for the slots the blocks with one pass fewer leave.  The
  // column jobs are four dependent rounds of loads per wave and nobody reads their sums before the update: with CA_VAR_GENE_RIDE they ride on the launch that
  // follows (k_poly_tail, or k_poly_red where the reduction keeps its launch) and yfin.ncol is 0 here; off, they stay as they were.
  if ((int)blockIdx.x >= ncb) {
    const int e = (int)blockIdx.x - ncb;
    const int ncolblk = (yfin.ncol + CA_TB / 64 - 1) / (CA_TB / 64);
    CA_LAB_CELL_EDGE(blockIdx.x, 0, e < ncolblk ? 3 : 2);
    if (e < ncolblk) {
      const int job = e * (CA_TB / 64) + (int)(threadIdx.x >> 6);
      if (job < yfin.ncol) ca_yfin_col_wave(yfin, job);
    } else if (e - ncolblk < yfin.nrow) {
      __shared__ double ca_yfin_sm[CA_TB / 64];
      ca_yfin_row_block(yfin, e - ncolblk, ca_yfin_sm);
    }
    CA_LAB_CELL_EDGE_END(blockIdx.x);
    return;
  }
  CA_LAB_CELL_EDGE(blockIdx.x, 0, 1);
  constexpr int CPB = CA_TB / CP;             // cells per pass of the block
  constexpr int RQ = R + 2;                   // moments 0 .. R + 1 (the derivative of q needs one more)
  constexpr int NBR = 4;                      // bins whose moments a thread keeps in registers (the usual case: one to three bins); the rest go through its slab
  __shared__ double sm[CA_TB];
  __shared__ double la[64];
  __shared__ double s_eb[CPB][NB];            // exp(x v_b)
  constexpr int NXK = (RQ + CP - 1) / CP;     // powers a lane keeps (LEAN): k = c, c + CP, ...
  constexpr int XS = LEAN ? NXK * CP : RQ;    // (LEAN: a row padded to whole rounds of the lane group, so that its stores need no bound; the padding is never read)
  __shared__ double s_xp[CPB][XS];            // x^k
  __shared__ double s_cf[CPB][8];             // coef
  // the coefficient tables of the first NBL bins (the usual case has one to three) in LDS: every pass of the block reads them again, 42 loads per lane and bin,
  // and from global memory those loads -- not the arithmetic -- were what a pass took
  constexpr int NBL = CA_PL_NBL;
  __shared__ double s_tb[NBL][(R + 1) * 16];
  static_assert(!EDGE || (LEAN && MFMA), "the head and block end of CA_VAR_CELL_EDGE exist for the lean MFMA form");
  using pre_t = typename std::conditional<LEAN, ca_cell_pre_lean, ca_cell_pre>::type;
  using x_t = typename std::conditional<LEAN, float, double>::type;
  [[maybe_unused]] x_t x_head = 0; [[maybe_unused]] pre_t pre_head = {};
  int nb_; [[maybe_unused]] double vlo_ = 0.0, delta_ = 0.0;
  if constexpr (EDGE) {
    // every load of the head before the first wait: alpha (wanted first), the header, the first pass's operands, the tables of all NBL bins (in bounds whatever nb:
    // the workspace holds NB of them; those past nb are staged and never read)
    const int t_ = threadIdx.x, c8 = t_ & 7;
    const float auf = alpha_u[c8 < C ? c8 : C - 1];
    nb_ = hdr->nb; vlo_ = hdr->vlo; delta_ = hdr->delta;
    if ((int64_t)blockIdx.x * CPB < N) {   // (blockIdx.x < ngroups: a block without a pass loads no cell)
      const int64_t n_ = (int64_t)blockIdx.x * CPB + t_ / CP, nn_ = n_ < N ? n_ : N - 1;
      const int cc_ = t_ % CP < C ? t_ % CP : C - 1;
      x_head = (x_t)p.F[nn_];
      pre_head.gl = p.glogit[nn_ * C + cc_]; pre_head.sn = p.s64[nn_]; pre_head.Anc = p.A[nn_ * C + cc_];
      pre_head.cn = p.cn[nn_];
    }
    constexpr int NST = (NBL < NB ? NBL : NB) * (R + 1) * 16, NSL = (NST + CA_TB - 1) / CA_TB;
    double stg[NSL];
#pragma unroll
    for (int j = 0; j < NSL; ++j) { const int i = j * CA_TB + t_; stg[j] = tabB[i < NST ? i : NST - 1]; }
    for (int i = t_; i < CPB * NB; i += CA_TB) (&s_eb[0][0])[i] = 0.0;   // (bins past nb: zeros, so that the gather needs no bounds)
    // log softmax(alpha), a copy per wave in la[8 wave ..]: lane groups of eight, one lane per clone; ca_log_softmax_alpha's additions (its butterfly pairs xor 1, 2, 4
    // first; lanes past C hold -inf / 0.0, so every later step compares with -inf or adds an exact 0.0)
    const double au = c8 < C ? (double)auf : -INFINITY;
    double mx = au;
    mx = fmax(mx, ca_dpp_xor<1>(mx)); mx = fmax(mx, ca_dpp_xor<2>(mx)); mx = fmax(mx, ca_dpp_xor<4>(mx));
    double se = c8 < C ? exp(au - mx) : 0.0;
    se += ca_dpp_xor<1>(se); se += ca_dpp_xor<2>(se); se += ca_dpp_xor<4>(se);
    if ((t_ & 63) < 8 && c8 < C) la[(t_ >> 6) * 8 + c8] = au - (mx + log(se));
#pragma unroll
    for (int j = 0; j < NSL; ++j) { const int i = j * CA_TB + t_; if (i < NST) (&s_tb[0][0])[i] = stg[j]; }
  } else {
  nb_ = hdr->nb;
  ca_log_softmax_alpha(alpha_u, C, la);
  for (int i = threadIdx.x; i < CPB * NB; i += CA_TB) (&s_eb[0][0])[i] = 0.0;   // (bins past nb: zeros, so that the gather needs no bounds)
  for (int i = threadIdx.x; i < (nb_ < NBL ? nb_ : NBL) * (R + 1) * 16; i += CA_TB) (&s_tb[0][0])[i] = tabB[i];
  }
  const int nb = nb_;
  __syncthreads();
  const int t = threadIdx.x, c = t % CP, slot = t / CP;
  double vlo, delta;
  if constexpr (EDGE) { vlo = vlo_; delta = delta_; } else { vlo = hdr->vlo; delta = hdr->delta; }
  // backward moments: thread t < (R + 2) C owns (k, clone) = (t / C, t % C) of EVERY bin -- nobody else adds to its outputs, cells are added in cell order
  const bool qown = t < RQ * C;
  const int qk = qown ? t / C : 0, qc = qown ? t % C : 0;
  [[maybe_unused]] double qa[NBR] = {0.0, 0.0, 0.0, 0.0};
  using qtile_t = __attribute__((ext_vector_type(4))) double;
  constexpr int BPT = 16 / CP;         // bins per column tile of the MFMA gather
  constexpr int NCT = NBR / BPT;       // its column tiles: bins 0 .. NBR - 1
  constexpr int KST = 64 / CP / 4;     // its steps per pass: four of the wave's cells each
  static_assert(CP == 4 || CP == 8, "the MFMA gather's column map");
  static_assert(CA_TB == 256, "four waves: each owns a quarter of a pass's cells, and the block's end adds four waves' tiles");
  [[maybe_unused]] qtile_t qm[2][NCT];
#pragma unroll
  for (int j = 0; j < NCT; ++j) { qm[0][j] = qtile_t{0.0, 0.0, 0.0, 0.0}; qm[1][j] = qtile_t{0.0, 0.0, 0.0, 0.0}; }
  const int wv = t >> 6, mrow = t & 15, mk = (t >> 4) & 3;   // the wave; this lane's row / column of a tile and its cell of a step
  const int mcl = mrow % CP, mbl = mrow / CP;                // the column's clone and bin inside its tile
  double* mine = Qpart + (int64_t)blockIdx.x * (NB * RQ * 8);
  if (qown) for (int b = NBR; b < nb; ++b) mine[(b * RQ + qk) * C + qc] = 0.0;
  ca_cell_acc acc = {0.0, 0.0, 0.0, 0.0, 0.0};
  const int64_t ngroups = (N + CPB - 1) / CPB;
  const int cc = c < C ? c : C - 1;
  // what the epilogue reads for this lane's (cell, clone) that nothing here produces: loaded a pass AHEAD, beside the arithmetic of the current one
  // (pre_t.  LEAN: x travels as the float it is, x_t, and widens at the top of its own pass -- widened beside its load, the prefetch was waited for where it was issued)
  auto load_pass = [&](int64_t grp, x_t& x_, pre_t& pre_) {
    const int64_t n_ = grp * CPB + slot, nn_ = n_ < N ? n_ : N - 1;
    x_ = (x_t)p.F[nn_];
    pre_.gl = p.glogit[nn_ * C + cc]; pre_.sn = p.s64[nn_]; pre_.Anc = p.A[nn_ * C + cc];
    if constexpr (LEAN) pre_.cn = p.cn[nn_];
  };
  x_t x_next = 0; pre_t pre_next = {};
  if constexpr (EDGE) { x_next = x_head; pre_next = pre_head; }   // (issued with the head's other loads)
  else if ((int64_t)blockIdx.x < ngroups) load_pass(blockIdx.x, x_next, pre_next);
  [[maybe_unused]] int pass = 0;   // (the timing lab's stamps)
  CA_LAB_CELL_EDGE(blockIdx.x, 1, 0);
  for (int64_t grp = blockIdx.x; grp < ngroups; grp += ncb, ++pass) {
    CA_LAB_CELL_PH(blockIdx.x, pass, 0);
    const int64_t n = grp * CPB + slot;
    const double x = (double)x_next; pre_t pre = pre_next;
    if constexpr (LEAN) pre.x = x;
    if (grp + ncb < ngroups) load_pass(grp + ncb, x_next, pre_next);
    double ZA = 0.0, ZB = 0.0, dZB = 0.0;
#define CA_PL_HORNER(TB)                                                  \
      pa = (TB)[R * 16 + cc]; pb = (TB)[R * 16 + 8 + cc];                 \
      _Pragma("unroll 10")                                                \
      for (int k = R - 1; k >= 0; --k) {                                  \
        dpb = dpb * x + pb;                                               \
        pa = pa * x + (TB)[k * 16 + cc];                                  \
        pb = pb * x + (TB)[k * 16 + 8 + cc];                              \
      }
#define CA_PL_BIN(b)                                                      \
    {                                                                     \
      const double vb = vlo + ((double)(b) + 0.5) * delta;                \
      const double e = exp(x * vb);                                       \
      double pa, pb, dpb = 0.0;                                           \
      if ((b) < NBL) { CA_PL_HORNER(s_tb[b]) }              /* (LDS) */   \
      else { const double* tb = tabB + ((int64_t)(b) * (R + 1)) * 16; CA_PL_HORNER(tb) } \
      ZA += e * pa; ZB += e * pb; dZB += e * (vb * pb + dpb);             \
      if (c == 0) s_eb[slot][b] = e;                                      \
    }
    [[maybe_unused]] ca_cell_qz qz;
    if constexpr (EDGE) {   // bin 0 (nb >= 1) as straight-line code, and beside it the q(z) half of the epilogue: it needs the prefetched logit alone
      qz = ca_cell_qz_half<CP>(pre.gl, n < N && c < C);
      CA_PL_BIN(0)
      for (int b = 1; b < nb; ++b) CA_PL_BIN(b)
    } else {
    for (int b = 0; b < nb; ++b) CA_PL_BIN(b)
    }
#undef CA_PL_BIN
#undef CA_PL_HORNER
    CA_LAB_CELL_PH_AFTER(dZB, blockIdx.x, pass, 1);
    if constexpr (LEAN) {   // x^k: every lane runs the chain, keeps its own k = c, c + CP, ... by selects and stores them without a condition
      double xk = 1.0, keep[NXK];
#pragma unroll
      for (int j = 0; j < NXK; ++j) keep[j] = 0.0;
#pragma unroll
      for (int k = 0; k < RQ; ++k) { keep[k / CP] = (k % CP == c) ? xk : keep[k / CP]; xk *= x; }
#pragma unroll
      for (int j = 0; j < NXK; ++j) s_xp[slot][j * CP + c] = keep[j];
    } else {   // x^k, the lanes of a cell sharing the stores
      double xk = 1.0;
      for (int k = 0; k < RQ; ++k) { if (k % CP == c) s_xp[slot][k] = xk; xk *= x; }
    }
    CA_LAB_CELL_PH(blockIdx.x, pass, 2);
    float cff = 0.f;
    if constexpr (EDGE) ca_cell_fused_group<CP, true, true, true>(p, la + (t >> 6) * 8 /* the wave's own copy */, n, N, C, 1, K, ZA, ZB, acc, &pre, &cff, &qz);
    else
    ca_cell_fused_group<CP, true, LEAN>(p, la, n, N, C, 1, K, ZA, ZB, acc, &pre, &cff);
    // this lane's coef as the epilogue stored it (float: what the matrix-core way back reads as well); d/dF = sum_c coef dZ/dx
    const double cf = (double)cff;
    double df = cf * dZB;
    if constexpr (LEAN) df = ca_dpp_gsum<CP>(df);
    else {
#pragma unroll
    for (int o = CP / 2; o > 0; o >>= 1) df += __shfl_xor(df, o, CP);
    }
    if (c == 0 && n < N) dF[n] = (float)df;
    if (c < 8) s_cf[slot][c] = cf;
    CA_LAB_CELL_PH_AFTER(df, blockIdx.x, pass, 3);
    if constexpr (MFMA) {
      // (the wave reads what its own lanes stored: the LDS serves one wave's operations in order, the fences keep the compiler from moving them)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
      for (int s = 0; s < KST; ++s) {
        const int cell = wv * (64 / CP) + s * 4 + mk;
        const double a0 = s_xp[cell][mrow];
        const double a1 = s_xp[cell][16 + mrow < XS ? 16 + mrow : XS - 1];   // (rows RQ .. 31 of the second tile are never stored: whatever they multiply)
        const double cfv = s_cf[cell][mcl];
#pragma unroll
        for (int j = 0; j < NCT; ++j) {
          if (j == 0 || nb > j * BPT) {   // (uniform: a column tile whose bins are all absent)
            const double bv = cfv * s_eb[cell][j * BPT + mbl];
            qm[0][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, bv, qm[0][j], 0, 0, 0);
            qm[1][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, bv, qm[1][j], 0, 0, 0);
          }
        }
      }
      if (nb > NBR) {   // (uniform; a wide exponent range: the thread's own words of its block's slab, all the pass's cells in cell order, as before)
        __syncthreads();
        if (qown) {
          for (int b = NBR; b < nb; ++b) {
            double a = mine[(b * RQ + qk) * C + qc];
            for (int s = 0; s < CPB; ++s) a += s_cf[s][qc] * s_xp[s][qk] * s_eb[s][b];
            mine[(b * RQ + qk) * C + qc] = a;
          }
        }
        __syncthreads();
      } else {          // (the next pass's stores behind this pass's loads: one wave, in order)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      }
      CA_LAB_CELL_PH_AFTER(qm[0][0][0], blockIdx.x, pass, 4);
      continue;
    }
    __syncthreads();
    CA_LAB_CELL_PH(blockIdx.x, pass, 4);
    if (qown) {
      // (loads batched eight cells at a time: a load per step waited for the one before, and that chain WAS this kernel; bins past nb hold zeros)
      if (nb == 1) {
#pragma unroll 8
        for (int s = 0; s < CPB; ++s) qa[0] += s_cf[s][qc] * s_xp[s][qk] * s_eb[s][0];
      } else {
#pragma unroll 8
        for (int s = 0; s < CPB; ++s) {
          const double w = s_cf[s][qc] * s_xp[s][qk];
          qa[0] += w * s_eb[s][0]; qa[1] += w * s_eb[s][1]; qa[2] += w * s_eb[s][2]; qa[3] += w * s_eb[s][3];
        }
      }
      for (int b = NBR; b < nb; ++b) {        // (a wide exponent range: the thread's own words of its block's slab, cell order all the same)
        double a = mine[(b * RQ + qk) * C + qc];
        for (int s = 0; s < CPB; ++s) a += s_cf[s][qc] * s_xp[s][qk] * s_eb[s][b];
        mine[(b * RQ + qk) * C + qc] = a;
      }
    }
    CA_LAB_CELL_PH_AFTER(qa[0], blockIdx.x, pass, 5);
    __syncthreads();
    CA_LAB_CELL_PH(blockIdx.x, pass, 6);
  }
  CA_LAB_CELL_EDGE(blockIdx.x, 2, 0);
  if constexpr (EDGE) {
    // The block end in one parking step.  Before any barrier every wave leaves what it owes where the passes never write: its three sums (the butterfly's
    // additions, ca_dpp_wave_sum) in la[32 ..], behind the four copies of log alpha, and its lanes' gamma sums in sm.  The first barrier says that every wave is
    // past its last pass, so the passes' arrays are idle: waves 1, 2, 3 park their tiles there.  Behind the second, wave 0 adds the tiles to its own (lane for lane
    // in the tile map, wave order) and stores the slab, and wave 1 makes the block sums of ca_cell_fused_finish -- waves 0, 1, 2, 3; cells 0 .. CPB - 1 from 0.0 --
    // its loads sixteen at a time in front of their adds.
    constexpr int QW = RQ * NBR * CP;   // one wave's tiles: [k][bin CP + clone]
    static_assert(CPB * NB >= QW && CPB * XS >= QW && NBL * (R + 1) * 16 >= QW, "a wave's tiles fit each of the three arrays");
    static_assert(32 + 3 * (CA_TB / 64) <= 64, "the waves' sums behind the copies of log alpha");
    const double r0 = ca_dpp_wave_sum(acc.ee), r1 = ca_dpp_wave_sum(acc.pr), r2 = ca_dpp_wave_sum(acc.q);
    if ((t & 63) == 0) { la[32 + 3 * wv + 0] = r0; la[32 + 3 * wv + 1] = r1; la[32 + 3 * wv + 2] = r2; }
    sm[t] = acc.gsumc;
    __syncthreads();
    double* const p1 = &s_eb[0][0], * const p2 = &s_xp[0][0], * const p3 = &s_tb[0][0];
    double* const pw = wv == 1 ? p1 : (wv == 2 ? p2 : p3);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < NCT; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int k = 16 * i + 4 * r + mk;
          if (wv > 0 && k < RQ) pw[k * (NBR * CP) + j * 16 + mrow] = qm[i][j][r];   // (column j 16 + mrow = bin CP + clone)
        }
    __syncthreads();
    if (wv == 0) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NCT; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int k = 16 * i + 4 * r + mk, col = j * 16 + mrow, b = j * BPT + mbl;
            if (k < RQ && b < nb && mcl < C) mine[(b * RQ + k) * C + mcl] = ((qm[i][j][r] + p1[k * (NBR * CP) + col]) + p2[k * (NBR * CP) + col]) + p3[k * (NBR * CP) + col];
          }
    } else if (wv == 1) {
      const int l = t & 63, W_ = 3 + C;
      if (l < C) {
        double a = 0.0;
#pragma unroll
        for (int i0 = 0; i0 < CPB; i0 += 16) {   // (sixteen loads, then their adds: cells 0 .. CPB - 1 in order)
          double g[16];
#pragma unroll
          for (int i = 0; i < 16; ++i) g[i] = sm[(i0 + i) * CP + l];
#pragma unroll
          for (int i = 0; i < 16; ++i) a += g[i];
        }
        cell_part[(int64_t)blockIdx.x * W_ + 3 + l] = a;
      } else if (l >= 8 && l < 11) {
        const double w0 = la[32 + l - 8], w1 = la[35 + l - 8], w2 = la[38 + l - 8], w3 = la[41 + l - 8];
        cell_part[(int64_t)blockIdx.x * W_ + l - 8] = ((w0 + w1) + w2) + w3;
      }
    }
    CA_LAB_CELL_EDGE_END(blockIdx.x);
    return;
  }
  ca_cell_fused_finish<CP>(acc, sm, cell_part, blockIdx.x, C);
  if constexpr (MFMA) {   // the four waves' tiles, added in wave order, into the block's slab
    // Waves 1, 2, 3 park theirs in LDS arrays of the passes, which nobody reads any more (every wave is past the barriers of ca_cell_fused_finish, so past its
    // last pass); wave 0 adds them to its own, lane for lane in the tile map, and stores the sums.  No LDS of its own: the launch's extra blocks pay for none.
    constexpr int QW = RQ * NBR * CP;   // one wave's tiles: [k][bin CP + clone]
    static_assert(CPB * NB >= QW && CPB * XS >= QW && NBL * (R + 1) * 16 >= QW, "a wave's tiles fit each of the three arrays");
    double* const p1 = &s_eb[0][0], * const p2 = &s_xp[0][0], * const p3 = &s_tb[0][0];
    double* const pw = wv == 1 ? p1 : (wv == 2 ? p2 : p3);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < NCT; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int k = 16 * i + 4 * r + mk;
          if (wv > 0 && k < RQ) pw[k * (NBR * CP) + j * 16 + mrow] = qm[i][j][r];   // (column j 16 + mrow = bin CP + clone)
        }
    __syncthreads();
    if (wv == 0) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NCT; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int k = 16 * i + 4 * r + mk, col = j * 16 + mrow, b = j * BPT + mbl;
            if (k < RQ && b < nb && mcl < C) mine[(b * RQ + k) * C + mcl] = ((qm[i][j][r] + p1[k * (NBR * CP) + col]) + p2[k * (NBR * CP) + col]) + p3[k * (NBR * CP) + col];
          }
    }
  } else if (qown) {
#pragma unroll
    for (int b = 0; b < NBR; ++b) if (b < nb) mine[(b * RQ + qk) * C + qc] = qa[b];
  }
  CA_LAB_CELL_EDGE_END(blockIdx.x);
}

// ---- fixed-order sums of the block partials: one wave per output, lanes stride over the blocks, then the wave's tree (same order every time) --------
// mode 0: plain sum (tabB); mode 1: sum / k! with k = (j / C) % (R + 2) (tabQ = Q_k / k!)
// this rank's max |x| into its slot, zeros into the other ranks' (the body of k_poly_xslot; also rides on the reduction launch of the backward moments)
struct ca_xslot_args { const float* xpart; int nx; const float* F; int64_t N; double* slots; int rank, world; };
__device__ __forceinline__ void ca_poly_xslot_body(const ca_xslot_args& a) {
  __shared__ float sx[CA_TB / 64];
  float ax = 0.f;
  if (a.nx > 0) { for (int i = threadIdx.x; i < a.nx; i += CA_TB) ax = fmaxf(ax, a.xpart[i]); }
  else { for (int64_t i = threadIdx.x; i < a.N; i += CA_TB) { const float v = fabsf(a.F[i]); ax = fmaxf(ax, v == v ? v : INFINITY); } }
  ax = warp_max(ax);
  if ((threadIdx.x & 63) == 0) sx[threadIdx.x >> 6] = ax;
  __syncthreads();
  if ((int)threadIdx.x < a.world) a.slots[threadIdx.x] = (int)threadIdx.x == a.rank ? (double)fmaxf(fmaxf(sx[0], sx[1]), fmaxf(sx[2], sx[3])) : 0.0;
}
// (nred: the blocks that reduce; a cell-sharded fit adds two more behind them -- the pending monitor pass's local block sums (a ca_small_args with
//  reduce_only) and this rank's max |x| slot -- what would otherwise be two small launches in front of the iteration's collective.  Behind those `nfix` blocks:
//  the count-matrix stream's column jobs, four to a block, where the reduction keeps a launch of its own and CA_VAR_GENE_RIDE moves them off the cell launch --
//  a cell-sharded fit, whose collective carries their sums.  COLS = false: no such jobs -- the forward moments' reduction, and every reduction with the switch
//  off: the launch as it was, registers and all; the column waves' 32 loads in flight per lane are compiled into the form that runs them only)
template <bool COLS>
__global__ void __launch_bounds__(CA_TB) k_poly_red(const double* __restrict__ part, int nblk, int64_t stride, const ca_poly_hdr* __restrict__ hdr, int per_bin,
                                                    int mode, int C, double* __restrict__ out, unsigned int* __restrict__ xbits, int nred, ca_small_args tail,
                                                    ca_xslot_args xs, int nfix, ca_yfin_args yfin) {
  if ((int)blockIdx.x >= nred) {
    const int e = (int)blockIdx.x - nred;
    if (COLS && e >= nfix) {
      if constexpr (COLS) {
        const int job = (e - nfix) * (CA_TB / 64) + (int)(threadIdx.x >> 6);
        if (job < yfin.ncol) ca_yfin_col_wave(yfin, job);
      }
    }
    else if (e == 0 && tail.enabled) ca_final_small_body(tail);
    else if (xs.slots) ca_poly_xslot_body(xs);
    return;
  }
  if (xbits && blockIdx.x == 0 && threadIdx.x == 0) *xbits = 0u;   // (its reader, k_poly_B, is complete: ready for the next state's maximum)
  ca_pm_red_body<false>(part, nblk, stride, hdr->nb * per_bin, mode, C, out, blockIdx.x * (CA_TB / 64) + (threadIdx.x >> 6), nred * (CA_TB / 64));
}

#include "ca_polygene.hip.h"    // the per-gene body, and the launch that runs reduction, per-gene pass, monitor tail and column jobs as one grid (CA_VAR_GENE_RIDE)

// ---- K3: per gene: the two gradient sums from its bin's polynomial (ca_pg_gene_block), as a launch of its own behind k_poly_red ---------------------------------
__global__ void __launch_bounds__(CA_TB) k_poly_gene(const ca_poly_hdr* __restrict__ hdr, const double* __restrict__ tabQ, const float* __restrict__ V,
                                                     const float* __restrict__ mu, const float* __restrict__ Lb, int G, int C,
                                                     double* __restrict__ red_g /*[G][2]: d/dmu, d/dV*/, ca_small_args tail, int ngblk) {
  if ((int)blockIdx.x >= ngblk) {   // a pending monitor pass's tail (cell partials -> red, psi.(YW) sum, ELBO assembly): the extra block, as on the matrix-core way back
    if (tail.enabled) ca_final_small_body(tail);
    return;
  }
  __shared__ double s_tq[CA_PL_NBL][(R + 2) * 8];
  ca_pg_gene_block<false>(hdr, tabQ, V, mu, Lb, G, C, red_g, (int)blockIdx.x, s_tq, nullptr, nullptr);
}

inline int cdiv_i(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

}  // namespace ca_series
using namespace ca_series;

size_t ca_poly_workspace_bytes(int G, int n_cell_blocks) {
  const size_t nbg = (size_t)cdiv_i(G, GPB);
  return sizeof(ca_poly_hdr) + 64 + ((nbg * sizeof(unsigned int) + 63) / 64) * 64 + CA_PL_NGFLAG * sizeof(unsigned int) + sizeof(double) * ((size_t)NB * (R + 1) * 16 * (nbg + 1) + (size_t)NB * (R + 2) * 8 * ((size_t)n_cell_blocks + 1));
}

void ca_poly_bind(ca_poly_ws* w, void* base, int G, int n_cell_blocks) {
  char* q = static_cast<char*>(base);
  w->hdr = reinterpret_cast<ca_poly_hdr*>(q); q += sizeof(ca_poly_hdr);
  w->xbits = reinterpret_cast<unsigned int*>(q); q += 64;
  const size_t nbg = (size_t)cdiv_i(G, GPB);
  w->mflags = reinterpret_cast<unsigned int*>(q); q += ((nbg * sizeof(unsigned int) + 63) / 64) * 64;   // (the moment role's tags, ca_polymom.hip.h: zeroed with the workspace)
  w->gflags = reinterpret_cast<unsigned int*>(q); q += CA_PL_NGFLAG * sizeof(unsigned int);   // (the merged way back's tags, ca_polygene.hip.h: likewise)
  w->tabB = reinterpret_cast<double*>(q); q += sizeof(double) * (size_t)NB * (R + 1) * 16;
  w->partB = reinterpret_cast<double*>(q); q += sizeof(double) * (size_t)NB * (R + 1) * 16 * nbg;
  w->tabQ = reinterpret_cast<double*>(q); q += sizeof(double) * (size_t)NB * (R + 2) * 8;
  w->Qpart = reinterpret_cast<double*>(q);
  w->n_cell_blocks = n_cell_blocks; w->n_gene_blocks = (int)nbg;
}

// a cell-sharded fit: this rank's max |x| of the CURRENT state into its slot of `slots[world]`, zeros into the others -- the sum over the ranks (the fit's one collective
// per iteration carries the slots) then holds every rank's maximum.  One block; from the merged update's per-piece maxima where they are current, else from F.
__global__ void __launch_bounds__(CA_TB) k_poly_xslot(const float* __restrict__ xpart, int nx, const float* __restrict__ F, int64_t N, double* __restrict__ slots, int rank,
                                                      int world) {
  const ca_xslot_args a = {xpart, nx, F, N, slots, rank, world};
  ca_poly_xslot_body(a);
}
hipError_t ca_poly_xslot(hipStream_t st, const float* xpart, int nx, const float* F, int64_t N, double* slots, int rank, int world) {
  hipLaunchKernelGGL(k_poly_xslot, dim3(1), dim3(CA_TB), 0, st, xpart, xpart ? nx : 0, F, N, slots, rank, world);
  return hipGetLastError();
}

hipError_t ca_poly_ranges(hipStream_t st, const ca_poly_ws* w, const float* V, const float* F, int G, int64_t N, double* mirror, double seq, const float* xpart, int nx,
                          const double* xglob, int nglob, double xadd) {
  if (!xpart) nx = 0;
  if (!xglob) nglob = 0;
  if (nx == 0 && nglob == 0) hipLaunchKernelGGL(k_poly_xmax, dim3((unsigned)std::min<int64_t>(128, (N + 4 * CA_TB - 1) / (4 * CA_TB))), dim3(CA_TB), 0, st, F, N, w->xbits);
  hipLaunchKernelGGL(k_poly_ranges, dim3(1), dim3(CA_TB), 0, st, V, G, w->xbits, mirror, seq, xpart, nglob ? 0 : nx, xglob, nglob, xadd);
  return hipGetLastError();
}

hipError_t ca_poly_moments(hipStream_t st, const ca_poly_ws* w, const float* V, const float* F, const float* muA, const float* muB, const float* Lb, int G,
                           int64_t N, int C, unsigned int* bad_word, double* mirror, double seq, const float* xpart, int nx, const double* xglob, int nglob, double xadd) {
  if (!xpart) nx = 0;
  if (!xglob) nglob = 0;
  if (nx == 0 && nglob == 0) hipLaunchKernelGGL(k_poly_xmax, dim3((unsigned)std::min<int64_t>(128, (N + 4 * CA_TB - 1) / (4 * CA_TB))), dim3(CA_TB), 0, st, F, N, w->xbits);
  ca_pm_args a;
  memset(&a, 0, sizeof(a));
  a.V = V; a.xbits = w->xbits; a.muA = muA; a.muB = muB; a.Lb = Lb; a.G = G; a.C = C; a.hdr = w->hdr; a.part = w->partB; a.bad_word = bad_word; a.mirror = mirror; a.seq = seq;
  a.xpart = xpart; a.nx = nglob ? 0 : nx; a.xglob = xglob; a.nglob = nglob; a.xadd = xadd;
  hipLaunchKernelGGL(k_poly_B, dim3(w->n_gene_blocks), dim3(TB_B), 0, st, a);
  {
    ca_small_args no_tail; memset(&no_tail, 0, sizeof(no_tail));
    ca_xslot_args no_xs; memset(&no_xs, 0, sizeof(no_xs));
    ca_yfin_args no_yfin; memset(&no_yfin, 0, sizeof(no_yfin));
    hipLaunchKernelGGL(k_poly_red<false>, dim3(256), dim3(CA_TB), 0, st, w->partB, w->n_gene_blocks, (int64_t)NB * (R + 1) * 16, w->hdr,
                       (R + 1) * 16, 0, C, w->tabB, w->xbits, 256, no_tail, no_xs, 0, no_yfin);
  }
  return hipGetLastError();
}

hipError_t ca_poly_cells(hipStream_t st, const ca_poly_ws* w, int64_t N, int C, int K, const void* cell_ptrs, const float* alpha_u, double* cell_part, float* dF,
                         const void* yfin_args, bool lean, bool mfma, bool edge) {
  const ca_cell_ptrs& p = *static_cast<const ca_cell_ptrs*>(cell_ptrs);
  ca_yfin_args yfin;
  if (yfin_args) memcpy(&yfin, yfin_args, sizeof(yfin)); else memset(&yfin, 0, sizeof(yfin));
  int CP = 1;
  while (CP < C) CP <<= 1;
  const int nextra = yfin_args ? cdiv_i(yfin.ncol, CA_TB / 64) + yfin.nrow : 0;
  const dim3 grid(w->n_cell_blocks + nextra);
#define CA_PCELL(CPV, LV) do { if (mfma) CA_PCELL_(CPV, LV, true); else CA_PCELL_(CPV, LV, false); } while (0)
#define CA_PCELL_(CPV, LV, MV) CA_PCELL__(CPV, LV, MV, false)
#define CA_PCELL__(CPV, LV, MV, EV) hipLaunchKernelGGL((k_poly_cell<CPV, LV, MV, EV>), grid, dim3(CA_TB), 0, st, w->hdr, w->tabB, p, alpha_u, cell_part, N, C, K, dF, w->Qpart, \
                                         w->n_cell_blocks, yfin)
  if (edge && !(lean && mfma)) return hipErrorInvalidValue;   // (the form exists for the lean MFMA launch: the engine asks for it nowhere else)
  if (lean) {   // (3 .. 8 clones: ca_poly_ok)
    if (K > 1) return hipErrorInvalidValue;   // (the lean epilogue takes psi of the prior term from x: one latent dimension, which is all ca_poly_ok admits)
    if (edge) { if (CP == 4) CA_PCELL__(4, true, true, true); else CA_PCELL__(8, true, true, true); }
    else
    if (CP == 4) CA_PCELL(4, true); else CA_PCELL(8, true);
  } else {
    if (CP == 4) CA_PCELL(4, false); else CA_PCELL(8, false);
  }
#undef CA_PCELL
#undef CA_PCELL_
#undef CA_PCELL__
  return hipGetLastError();
}

constexpr int NRED_Q = 256;   // reducer blocks of the backward moments: a wave per output, up to NB (R + 2) 8 = 5632 of them

hipError_t ca_poly_reduce(hipStream_t st, const ca_poly_ws* w, int64_t N, int C, const void* yfin_cols, const void* local_tail, const float* xs_part, int xs_n,
                          const float* xs_F, double* xs_slots, int rank, int world) {
  ca_small_args tail;
  if (local_tail) memcpy(&tail, local_tail, sizeof(tail)); else memset(&tail, 0, sizeof(tail));
  ca_yfin_args yfin;
  if (yfin_cols) memcpy(&yfin, yfin_cols, sizeof(yfin)); else memset(&yfin, 0, sizeof(yfin));
  yfin.nrow = 0;
  const ca_xslot_args xs = {xs_part, xs_part ? xs_n : 0, xs_F, N, xs_slots, rank, world};
  const int nfix = (tail.enabled || xs_slots) ? 2 : 0;
  if (yfin.ncol > 0)
    hipLaunchKernelGGL(k_poly_red<true>, dim3(NRED_Q + nfix + cdiv_i(yfin.ncol, CA_TB / 64)), dim3(CA_TB), 0, st, w->Qpart, w->n_cell_blocks, (int64_t)NB * (R + 2) * 8,
                       w->hdr, (R + 2) * C, 1, C, w->tabQ, nullptr, NRED_Q, tail, xs, nfix, yfin);
  else   // (no column jobs: the launch as it was)
    hipLaunchKernelGGL(k_poly_red<false>, dim3(NRED_Q + nfix), dim3(CA_TB), 0, st, w->Qpart, w->n_cell_blocks, (int64_t)NB * (R + 2) * 8, w->hdr,
                       (R + 2) * C, 1, C, w->tabQ, nullptr, NRED_Q, tail, xs, nfix, yfin);
  return hipGetLastError();
}

hipError_t ca_poly_backward(hipStream_t st, const ca_poly_ws* w, const float* V, const float* mu, const float* Lb, int G, int C, double* red_g, const void* small_tail) {
  ca_small_args tail;
  static_assert(sizeof(ca_small_args) <= 512, "ca_small_args");
  if (small_tail) memcpy(&tail, small_tail, sizeof(tail)); else memset(&tail, 0, sizeof(tail));
  const int ngblk = cdiv_i(G, CA_TB);
  hipLaunchKernelGGL(k_poly_gene, dim3(ngblk + (tail.enabled ? 1 : 0)), dim3(CA_TB), 0, st, w->hdr, w->tabQ, V, mu, Lb, G, C, red_g, tail, ngblk);
  return hipGetLastError();
}

hipError_t ca_poly_backward_merged(hipStream_t st, const ca_poly_ws* w, const float* V, const float* mu, const float* Lb, int G, int C, double* red_g,
                                   const void* small_tail, const void* yfin_cols, int nb_hint, unsigned int tag, unsigned long long timeout_ticks, unsigned int* err) {
  if (tag == 0u || !err) return hipErrorInvalidValue;
  ca_small_args tail;
  if (small_tail) memcpy(&tail, small_tail, sizeof(tail)); else memset(&tail, 0, sizeof(tail));
  ca_yfin_args yfin;
  if (yfin_cols) memcpy(&yfin, yfin_cols, sizeof(yfin)); else memset(&yfin, 0, sizeof(yfin));
  yfin.nrow = 0;
  ca_gr_args a;
  memset(&a, 0, sizeof(a));
  a.part = w->Qpart; a.nblk = w->n_cell_blocks; a.stride = (int64_t)NB * (R + 2) * 8; a.tabQ = w->tabQ;
  // (as many reducer blocks as nb_hint bins' outputs fill, a wave each; the waves stride over the outputs, so a bin count above the hint costs time, not outputs)
  a.nred = nb_hint > 0 ? std::min(NRED_Q, std::max(1, cdiv_i((int64_t)nb_hint * (R + 2) * C, CA_TB / 64))) : NRED_Q;
  a.hdr = w->hdr; a.V = V; a.mu = mu; a.Lb = Lb; a.G = G; a.C = C; a.red_g = red_g; a.ngblk = cdiv_i(G, CA_TB);
  a.flags = w->gflags; a.tag = tag; a.timeout_ticks = timeout_ticks; a.err = err;
  static_assert(NRED_Q <= CA_PL_NGFLAG, "a flag word per reducer block");
  // block order = dispatch order: reducers, gene blocks, the monitor pass's tail, the column jobs
  hipLaunchKernelGGL(k_poly_tail, dim3(a.nred + a.ngblk + (tail.enabled ? 1 : 0) + cdiv_i(yfin.ncol, CA_TB / 64)), dim3(CA_TB), 0, st, a, tail, yfin);
  return hipGetLastError();
}

#ifdef CA_LAB   // timing-lab builds only: reader of the cell passes' phase stamps (tools/lab/ca_lab_hooks.inc, tools/cell_stamps.py)
extern "C" int ca_lab_read_cell_stamps(unsigned long long* out, int n_words) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(ca_series::ca_lab_stamps4), (size_t)n_words * sizeof(unsigned long long)) == hipSuccess ? 0 : 2;
}
// ... and of the block-level stamps of every block of the cell launch (tools/cell_edges.py)
extern "C" int ca_lab_read_cell_edges(unsigned long long* out, int n_words) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(ca_series::ca_lab_stamps5), (size_t)n_words * sizeof(unsigned long long)) == hipSuccess ? 0 : 2;
}
#endif
