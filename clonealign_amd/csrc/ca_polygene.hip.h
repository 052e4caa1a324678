// ca_polygene.hip.h -- the series form's way back: the per-gene pass as a device body that two launches share, and the launch that runs the
// reduction of the backward moments, the per-gene pass, the pending monitor pass's tail and the count-matrix stream's column sums as ONE grid (CA_VAR_GENE_RIDE):
//   * k_poly_gene (ca_poly.hip): the per-gene pass as a launch of its own behind k_poly_red -- the two-launch order, kept for cell-sharded fits (the iteration's
//     collective sits between the two) and for the switch off;
//   * k_poly_tail (here): blocks [0, nred) reduce the cell launch's slabs into tabQ exactly as k_poly_red does in mode 1 (the same wave sums the same output), blocks
//     [nred, nred + ngblk) are the gene blocks, then one block for the monitor pass's tail where one is pending, then the stream's column jobs, four to a block.
// As two launches the reduction (5.6 us) and the per-gene pass (7.8 us) were two chains of dependent round trips with a kernel boundary between them on an idle
// device, about 1 us of fp64 arithmetic each.  In one grid a gene block has its loads of V, L, mu and the header, its bin and (v - v_b) behind it when the table arrives.
//
// Hand-over (the idiom of ca_polymom.hip.h, which argues it in full): a reducer stores its outputs with device-scope (write-through) stores, every wave waits until
// its stores are acknowledged (s_waitcnt vmcnt(0)), the block meets at its barrier and thread 0 stores this launch's tag into the block's flag word.  A gene block
// polls the flag words of the reducers that HAVE outputs -- the first ceil(nb (R + 2) C / 4) of them: the header's nb is an earlier launch's, both sides read the same
// number -- with relaxed device-scope loads, passes one device-scope acquire fence and its barrier, and reads tabQ with device-scope loads (into LDS, or past NBL bins
// from memory in the Horner steps themselves).  A reducer without an output stores nothing and nobody waits for it.
//   Why the wait ends: every block a gene block waits for has a lower index, depends on nobody in this launch (its slabs are the cell launch's) and runs to its flag
//   store once dispatched; the grid is a few hundred blocks on a device with room for two thousand, so in practice all of it is resident from the start, but the
//   argument needs only that a block which depends on nobody gets a slot.  The tail block and the column blocks wait for nobody and nobody waits for them.
//   The wait is bounded all the same (timeout_ticks of the s_memrealtime clock): on expiry the block stores the sticky error word and leaves -- red_g keeps what it
//   held -- and the host reports CA_ERR_STATE at its next synchronisation (comm_check).
//   The tag is per launch and never zero; the flag words live in the series workspace, zeroed at create, and are no other launch's.
#pragma once
#include "ca_poly.h"

struct ca_gr_args {
  // the reduction (k_poly_red's arguments in mode 1)
  const double* part; int nblk; int64_t stride; double* tabQ; int nred;
  // the per-gene pass (k_poly_gene's)
  const ca_poly_hdr* hdr; const float* V; const float* mu; const float* Lb; int G, C; double* red_g; int ngblk;
  // the hand-over
  unsigned int* flags;               // [nred] this launch's tag once the block's outputs are published
  unsigned int tag;                  // never 0
  unsigned long long timeout_ticks;  // bound of a gene block's wait (s_memrealtime, 100 MHz)
  unsigned int* err;                 // mapped host word: set when a wait ran out
};

struct ca_pg_dev_tab {   // tabQ behind the hand-over: every element by a device-scope load
  const double* p;
  __device__ __forceinline__ double operator[](int i) const {
    return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long*>(p + i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  }
};

// ---- per gene: the two gradient sums from its bin's polynomial; gene block `gblk` of a CA_TB-thread launch -----------------------------------------------------
// The moment tables of the first NBL bins (the usual case has one to three) in LDS: a gene reads 176 doubles of its bin's table, and from global memory that
// was a chain of 320 dependent-latency loads per thread -- the 11.9 us this launch took.  One load per step: T_{k+1} of a step is T_k of the one before.
// RIDE = false: tabQ is an earlier launch's, staged first.  RIDE = true (k_poly_tail): everything that does not need tabQ first, then the wait for the reducers' tags,
// then the same staging and the same Horner steps: every sum keeps its operands and its order.
template <bool RIDE>
__device__ __forceinline__ void ca_pg_gene_block(const ca_poly_hdr* __restrict__ hdr, const double* __restrict__ tabQ, const float* __restrict__ V,
                                                 const float* __restrict__ mu, const float* __restrict__ Lb, int G, int C, double* __restrict__ red_g, int gblk,
                                                 double (*s_tq)[(CA_PL_R + 2) * 8], [[maybe_unused]] const ca_gr_args* ride, [[maybe_unused]] int* s_gave_up) {
  constexpr int R = CA_PL_R, RQ = R + 2, NBL = CA_PL_NBL;
  const int t = threadIdx.x;
  const int nb = hdr->nb;
  const double vlo = hdr->vlo, delta = hdr->delta;
  if constexpr (!RIDE) {
    for (int i = t; i < (nb < NBL ? nb : NBL) * RQ * C; i += CA_TB) s_tq[i / (RQ * C)][i % (RQ * C)] = tabQ[i];
    __syncthreads();
  }
  const int g = gblk * CA_TB + t;
  const bool live = g < G;
  if constexpr (!RIDE) { if (!live) return; }
  const int gg = live ? g : G - 1;   // (RIDE: a thread past the last gene stays for the barriers and stores nothing)
  const double v = (double)V[gg];
  int b = (int)floor((v - vlo) / delta);
  b = b < 0 ? 0 : (b >= nb ? nb - 1 : b);
  const double dv = v - (vlo + ((double)b + 0.5) * delta);
  float lrow[8];
  {
    const float4 l0 = *reinterpret_cast<const float4*>(Lb + (int64_t)gg * CA_CW), l1 = *reinterpret_cast<const float4*>(Lb + (int64_t)gg * CA_CW + 4);
    lrow[0] = l0.x; lrow[1] = l0.y; lrow[2] = l0.z; lrow[3] = l0.w; lrow[4] = l1.x; lrow[5] = l1.y; lrow[6] = l1.z; lrow[7] = l1.w;
  }
  [[maybe_unused]] float mug = 0.f;
  if constexpr (RIDE) {
    mug = mu[gg];
    // the reducers that have an output: all of lower index, each runs to its flag store once dispatched (the header's argument)
    const int nout = nb * RQ * C, nw = CA_TB / 64;
    const int need = min(ride->nred, (nout + nw - 1) / nw);
    if (t == 0) *s_gave_up = 0;
    __syncthreads();
    {
      const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
      for (int i = t; i < need; i += CA_TB) {
        while (__hip_atomic_load(ride->flags + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != ride->tag) {
          if (__builtin_amdgcn_s_memrealtime() - t0 > ride->timeout_ticks) {
            __hip_atomic_store(ride->err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            *s_gave_up = 1;
            break;
          }
          __builtin_amdgcn_s_sleep(2);
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // nothing read from here on comes from a line cached before the tags were seen
    __syncthreads();
    if (*s_gave_up) return;   // (uniform: the sticky word is set, red_g keeps what it held, the host reports CA_ERR_STATE)
    const ca_pg_dev_tab tq = {tabQ};
    for (int i = t; i < (nb < NBL ? nb : NBL) * RQ * C; i += CA_TB) s_tq[i / (RQ * C)][i % (RQ * C)] = tq[i];
    __syncthreads();
    if (!live) return;
  }
  double s0 = 0.0, s1 = 0.0;
  // q = sum_{k <= R} dv^k T_k;  q' = sum_{k <= R} dv^k (k + 1) T_{k+1}   (T_k = Q_k / k!)
#define CA_PL_GENE(TQ)                                                            \
  _Pragma("unroll")                                                               \
  for (int c = 0; c < 8; ++c) {                                                   \
    if (c < C) {                                                                  \
      double tn = (TQ)[(R + 1) * C + c], tk = (TQ)[R * C + c];                    \
      double q = tk, dq = (double)(R + 1) * tn;                                   \
      _Pragma("unroll 10")                                                        \
      for (int k = R - 1; k >= 0; --k) {                                          \
        tn = tk; tk = (TQ)[k * C + c];                                            \
        q = q * dv + tk;                                                          \
        dq = dq * dv + (double)(k + 1) * tn;                                      \
      }                                                                           \
      const double l = (double)lrow[c];                                           \
      s0 += l * q; s1 += l * dq;                                                  \
    }                                                                             \
  }
  if (nb <= NBL) { CA_PL_GENE(s_tq[b]) }   // (uniform)
  else if constexpr (RIDE) { const ca_pg_dev_tab tq = {tabQ + (int64_t)b * RQ * C}; CA_PL_GENE(tq) }
  else { const double* tq = tabQ + (int64_t)b * RQ * C; CA_PL_GENE(tq) }
#undef CA_PL_GENE
  red_g[(int64_t)g * 2 + 0] = s0;
  if constexpr (RIDE) red_g[(int64_t)g * 2 + 1] = (double)mug * s1;
  else red_g[(int64_t)g * 2 + 1] = (double)mu[g] * s1;
}

// ---- reduction, per-gene pass, monitor tail and column jobs in one grid (the header's account) ----------------------------------------------------------------
__global__ void __launch_bounds__(CA_TB) k_poly_tail(ca_gr_args a, ca_small_args tail, ca_yfin_args yfin) {
  const int blk = (int)blockIdx.x, t = threadIdx.x;
  if (blk < a.nred) {
    // a reducer: k_poly_red's sums, outputs wave0, wave0 + 4 nred, ... -- the same wave of the same block as there
    constexpr int nw = CA_TB / 64;
    const int nout = a.hdr->nb * (CA_PL_R + 2) * a.C;
    if (blk * nw >= nout) return;   // (uniform: none of this block's waves has an output; nobody waits for it)
    ca_pm_red_body<false, true>(a.part, a.nblk, a.stride, nout, 1, a.C, a.tabQ, blk * nw + (t >> 6), a.nred * nw);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every output was stored write-through: the wave waits until its own are acknowledged ...
    __syncthreads();                                    // ... every wave of the block has ...
    if (t == 0) __hip_atomic_store(a.flags + blk, a.tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ... and only then the block's tag
    return;
  }
  const int e = blk - a.nred;
  if (e < a.ngblk) {
    __shared__ double s_tq[CA_PL_NBL][(CA_PL_R + 2) * 8];
    __shared__ int s_gave_up;
    ca_pg_gene_block<true>(a.hdr, a.tabQ, a.V, a.mu, a.Lb, a.G, a.C, a.red_g, e, s_tq, &a, &s_gave_up);
    return;
  }
  // a pending monitor pass's tail (cell partials -> red, psi.(YW) sum, ELBO assembly) and the stream's column sums: their inputs are the cell launch's
  const int x = e - a.ngblk, ntail = tail.enabled ? 1 : 0;
  if (x < ntail) { ca_final_small_body(tail); return; }
  const int job = (x - ntail) * (CA_TB / 64) + (t >> 6);
  if (job < yfin.ncol) ca_yfin_col_wave(yfin, job);
}
